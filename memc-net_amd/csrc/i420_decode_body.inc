// i420_decode_body.inc -- the body of i420_decode (video_io.hip) and i420_decode_lp<T> (lp_video_io.hip), included inside
// each kernel: a gather over the PADDED extent.  Lane (frame, padded row, quad of padded columns) clamps its source
// coordinates (replicate padding), decodes, stores T(float32(byte) / 255) into the three planes and, for the pixels inside
// the frame, the RGB bytes.  Every element has one writer.  Expects the storage tag T and the kernel's parameters
// (i420, frames, h, w, rgb, planes, sf, sc, sr, pl, pt, hp, wp).
    int f, yp, xp0;
    if (!quad_of_lane(frames, hp, (wp + 3) / 4, f, yp, xp0)) return;
    const int count = min(4, wp - xp0);
    const int64_t ny = (int64_t)h * w, nc = (int64_t)(h / 2) * (w / 2);
    const uint8_t *Y = i420 + (int64_t)f * (ny + 2 * nc), *U = Y + ny, *V = U + nc;
    const int oy = yp - pt, sy = min(max(oy, 0), h - 1);
    const int ox0 = xp0 - pl;
    const uint8_t *yrow = Y + (int64_t)sy * w;
    const int64_t crow = (int64_t)(sy / 2) * (w / 2);
    const bool inside = ox0 >= 0 && ox0 + 3 < w && count == 4;     // four source columns, none clamped

    uint8_t yb[4];
    if (inside) {
        const u8x4 y4 = *reinterpret_cast<const u8x4u *>(yrow + ox0);
        for (int j = 0; j < 4; j++) yb[j] = y4[j];
    } else {
        for (int j = 0; j < 4; j++) yb[j] = yrow[min(max(ox0 + j, 0), w - 1)];     // j >= count: a valid address, unused
    }
    Rgb4Bytes q;
    for (int j = 0; j < 4; j++) {
        const int sx = min(max(ox0 + j, 0), w - 1);
        uint8_t px[3];
        mv::decode_pixel(yb[j], U[crow + sx / 2], V[crow + sx / 2], px);
        for (int c = 0; c < 3; c++) q.b[3 * j + c] = px[c];
    }
    if (planes) {
        typename T::elem *o = planes + f * sf + yp * sr + xp0;
        for (int c = 0; c < 3; c++, o += sc) {
            if (count == 4) {
                typename T::vec v;
                for (int j = 0; j < 4; j++) v[j] = T::narrow((float)q.b[3 * j + c] / 255.0f);
                *reinterpret_cast<typename T::vecu *>(o) = v;
            } else {
                for (int j = 0; j < count; j++) o[j] = T::narrow((float)q.b[3 * j + c] / 255.0f);
            }
        }
    }
    if (rgb && oy >= 0 && oy < h) {
        uint8_t *o = rgb + (((int64_t)f * h + oy) * w + ox0) * 3;
        if (inside) {
            store_rgb4(o, 4, q);
        } else {
            for (int j = 0; j < count; j++) {
                if (ox0 + j < 0 || ox0 + j >= w) continue;
                for (int c = 0; c < 3; c++) o[3 * j + c] = q.b[3 * j + c];
            }
        }
    }
