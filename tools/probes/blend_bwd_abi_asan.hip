// tools/probes/blend_bwd_abi_asan.hip -- the host code of the three blend backward entry points (memc_fi_abi.hpp parses
// caller-supplied descriptors) under AddressSanitizer and UBSan, stand-alone: the three translation units are included as
// they are, and each entry point is called with malformed, empty and uncovered descriptors from the case list of
// tests/test_satellite_abi_codes.py (one 2x3x8x16 call, mutated), never with a call that would enqueue.  CPU only: no
// device is touched, the data pointers are made-up addresses that the checks compare and never follow.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//       -Iinclude -Imemc-net_amd/csrc -o blend_bwd_abi_asan tools/probes/blend_bwd_abi_asan.hip && ./blend_bwd_abi_asan
//
// Prints one line per entry point and dtype combination and "clean" at the end; a wrong code or a sanitizer report ends
// it with a non-zero status.
#include "../../memc-net_amd/csrc/fi_blend_bwd_c3.hip"
#include "../../memc-net_amd/csrc/mx_fi_blend_bwd_c3.hip"
#include "../../memc-net_amd/csrc/lp_fi_blend_bwd_c3.hip"

#include <stdio.h>
#include <functional>
#include <vector>

namespace {

constexpr int N = 2, C = 3, H = 8, W = 16, TAPS = 16;
enum Kind { IMAGE, FLOW, TAP, OCC };
const Kind kKinds[8] = {IMAGE, FLOW, TAP, OCC, IMAGE, FLOW, TAP, OCC};

memc_tensor4 desc(int64_t n, int64_t c, int64_t h, int64_t w, uintptr_t data, int64_t row = 0)
{
    row = row ? row : w;
    return {(float *)data, {n, c, h, w}, {c * h * row, h * row, row, 1}};
}

struct Call {
    memc_tensor4 t[8];
    const memc_tensor4 *p[8];
};

// the fixture's build(): tap_off bytes on every taps pointer, 2 bytes on the pointer of tensor f32_off
Call build(int n = N, int c = C, int w = W, int taps = TAPS, int tap_off = 0, int f32_off = -1)
{
    Call k;
    for (int i = 0; i < 8; i++) {
        const int chans[4] = {c, 2, taps, 1};
        const uintptr_t data = 0x1000u * (i + 1) + (kKinds[i] == TAP ? tap_off : 0) + (i == f32_off ? 2 : 0);
        k.t[i] = desc(n, chans[kKinds[i]], H, w, n ? data : 0);
        k.p[i] = &k.t[i];
    }
    return k;
}

struct Case {
    const char *name;
    int want;
    Call call;
};

// f32: a tensor of the call that is stored as fp32 (its pointer moved by 2 bytes: not covered), or -1 (none, or -- the fp32
// library -- no alignment is tested and the call would enqueue)
std::vector<Case> cases(int f32)
{
    std::vector<Case> out;
    auto add = [&](const char *name, int want, Call k, std::function<void(Call &)> mutate = nullptr) {
        if (mutate) mutate(k);
        out.push_back({name, want, k});         // (run() points p at the copy's own descriptors)
    };
    add("batch=0", 0, build(0));
    for (int i = 0; i < 8; i++) {
        add("null", -1, build(), [i](Call &k) { k.p[i] = nullptr; });
        add("nodata", -1, build(), [i](Call &k) { k.t[i].data = nullptr; });
        add("wstride", -1, build(), [i](Call &k) { k.t[i].stride[3] = 2; });
        add("bigstride", -1, build(), [i](Call &k) { k.t[i].stride[0] = (int64_t)1 << 33; });
        add("negative size", -1, build(), [i](Call &k) { k.t[i].size[2] = -1; });
        for (int dim = 0; dim < 4; dim++)
            add("grow", -1, build(), [i, dim](Call &k) {
                int64_t s[4] = {k.t[i].size[0], k.t[i].size[1], k.t[i].size[2], k.t[i].size[3]};
                s[dim] += 1;
                k.t[i] = desc(s[0], s[1], s[2], s[3], (uintptr_t)k.t[i].data);
            });
    }
    for (int i = 4; i < 8; i++)
        add("rows", -1, build(), [i](Call &k) {
            k.t[i] = desc(k.t[i].size[0], k.t[i].size[1], H, W, (uintptr_t)k.t[i].data, W + 4);
        });
    add("taps=0", -1, build(N, C, W, 0));
    add("taps=15", -1, build(N, C, W, 15));
    add("C=4", 1, build(N, 4));
    add("W=4", 1, build(N, C, 4));
    add("W=10", 1, build(N, C, 10));
    add("W=18", 1, build(N, C, 18));
    add("taps=8", -1, build(N, C, W, 8));      // (the exact rule: 8 taps have no side)
    add("taps=25", 1, build(N, C, W, 25));
    add("null & C=4", -1, build(N, 4), [](Call &k) { k.p[7] = nullptr; });
    add("taps=15 & W=10", -1, build(N, C, 10, 15));
    if (f32 >= 0) add("f32ptr+2", 1, build(N, C, W, TAPS, 0, f32));
    return out;
}

int failures = 0;

template <class F>
void run(const char *entry, int f32, bool half_taps, F call)
{
    std::vector<Case> cs = cases(f32);
    if (half_taps) cs.push_back({"tapptr+4", 1, build(N, C, W, TAPS, 4)});
    for (Case &c : cs) {
        for (int i = 0; i < 8; i++)
            if (c.call.p[i]) c.call.p[i] = &c.call.t[i];
        const int got = call(c.call.p);
        if (got != c.want) {
            printf("%s %s: returned %d, expected %d\n", entry, c.name, got, c.want);
            failures++;
        }
    }
    printf("%-44s %3zu calls\n", entry, cs.size());
}

}  // namespace

int main()
{
    run("blend_grad.bwd", -1, false, [](const memc_tensor4 *const *p) {
        return FilterInterpolationBlendLayer_gpu_backward(nullptr, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7]);
    });
    const memc_dtype half[2] = {MEMC_F16, MEMC_BF16};
    char label[64];
    for (memc_dtype t : half)
        for (memc_dtype ft : {MEMC_F32, t}) {
            snprintf(label, sizeof label, "mx_blend_grad.bwd %d,%d", (int)t, (int)ft);
            run(label, ft == MEMC_F32 ? 1 : 4, true, [=](const memc_tensor4 *const *p) {
                return FilterInterpolationBlendLayer_gpu_backward_mx(nullptr, t, ft, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7]);
            });
            for (memc_dtype gt : {MEMC_F32, t}) {
                snprintf(label, sizeof label, "lp_blend_grad.bwd %d,%d,%d", (int)t, (int)ft, (int)gt);
                run(label, ft == MEMC_F32 ? 5 : gt == MEMC_F32 ? 4 : -1, true, [=](const memc_tensor4 *const *p) {
                    return FilterInterpolationBlendLayer_gpu_backward_lp(nullptr, t, ft, gt, p[0], p[1], p[2], p[3], p[4], p[5],
                                                                         p[6], p[7]);
                });
            }
        }
    // dtype arguments the entry points refuse before they look at a descriptor (all NULL here)
    const memc_tensor4 *none[8] = {};
    auto expect = [](const char *what, int got) {
        if (got != -1) {
            printf("%s: returned %d, expected -1\n", what, got);
            failures++;
        }
    };
    expect("mx dtypes 0,0", FilterInterpolationBlendLayer_gpu_backward_mx(nullptr, MEMC_F32, MEMC_F32, none[0], none[1], none[2],
                                                                          none[3], none[4], none[5], none[6], none[7]));
    expect("lp dtypes 1,2,0", FilterInterpolationBlendLayer_gpu_backward_lp(nullptr, MEMC_F16, MEMC_BF16, MEMC_F32, none[0], none[1],
                                                                            none[2], none[3], none[4], none[5], none[6], none[7]));
    expect("lp dtypes 3,0,0", FilterInterpolationBlendLayer_gpu_backward_lp(nullptr, (memc_dtype)3, MEMC_F32, MEMC_F32, none[0],
                                                                            none[1], none[2], none[3], none[4], none[5], none[6],
                                                                            none[7]));
    printf(failures ? "%d wrong codes\n" : "clean\n", failures);
    return failures ? 1 : 0;
}
