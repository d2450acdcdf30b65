// rgb_quantise_body.inc -- the body of rgb_quantise (video_io.hip) and rgb_quantise_lp<T> (lp_video_io.hip), included inside
// each kernel: three quads of T in, twelve bytes out, mv::quantise on the exactly widened value.  Expects the storage tag T
// and the kernel's parameters (planes, sf, sc, sr, frames, h, w, rgb).
    int f, y, x0;
    if (!quad_of_lane(frames, h, (w + 3) / 4, f, y, x0)) return;
    const int count = min(4, w - x0);
    const typename T::elem *p = planes + f * sf + y * sr + x0;
    Rgb4Bytes q;
    q.v = u32x3{0u, 0u, 0u};
    for (int c = 0; c < 3; c++, p += sc) {
        if (count == 4) {
            const typename T::vec v = *reinterpret_cast<const typename T::vecu *>(p);
            for (int j = 0; j < 4; j++) q.b[3 * j + c] = mv::quantise(T::widen(v[j]));
        } else {
            for (int j = 0; j < count; j++) q.b[3 * j + c] = mv::quantise(T::widen(p[j]));
        }
    }
    store_rgb4(rgb + (((int64_t)f * h + y) * w + x0) * 3, count, q);
