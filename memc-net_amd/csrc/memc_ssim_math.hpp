// memc_ssim_math.hpp -- the per-window arithmetic of ssim.hip (libmemc_hip_ssim.so): skimage's compare_ssim at its defaults
// for two uint8 planes (7 x 7 uniform window, n = 49, sample covariance n / (n - 1), K1 = 0.01, K2 = 0.03, data range 255),
// restated on the window's five INTEGER sums.  Plain C++ that a host compiler takes as well (tests/test_ssim_abi.py runs it
// beside numpy on the host); networks/yuv_io.py::ssim_from_planes is the same expression in numpy.
//
// For a window with sums sx, sy (<= 12495) and sxx, syy, sxy (<= 3 186 225):
//   Vxx = 49 sxx - sx^2,  Vyy = 49 syy - sy^2,  Vxy = 49 sxy - sx sy            (|V| <= 255^2 * 600 = 39 015 000)
//   S = ((2 sx sy + c1) (2 Vxy + c2)) / ((sx^2 + sy^2 + c1) (Vxx + Vyy + c2))
//   c1 = (0.01 * 255)^2 * 49^2,  c2 = (0.03 * 255)^2 * 49 * 48
// which is skimage's map with numerator and denominator multiplied by 49^2 * (49 * 48).  Every integer term stays below
// 3.2e8: int32.  The integers convert to float64 exactly; then one add per factor, one multiply per factor pair and one
// division, nothing contracted or re-associated.  Equal windows give equal factors, so S == 1.0 exactly.
#ifndef MEMC_SSIM_MATH_HPP
#define MEMC_SSIM_MATH_HPP

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

#if defined(__HIPCC__)
#define MEMC_SSIM_FN __host__ __device__ __forceinline__
#else
#define MEMC_SSIM_FN inline
#endif

namespace memc_ssim {

constexpr int kWindow = 7;                           // the window's side; n = 49 samples
constexpr double kC1 = 0x1.e7e4051eb8520p+13;        // (0.01 * 255) ** 2 * 49 ** 2      = 15612.502500000002
constexpr double kC2 = 0x1.0cd675c28f5c2p+17;        // (0.03 * 255) ** 2 * 49 * 48      = 137644.91999999998

MEMC_SSIM_FN double window_ssim(int sx, int sy, int sxx, int syy, int sxy)
{
    const int vxx = 49 * sxx - sx * sx, vyy = 49 * syy - sy * sy, vxy = 49 * sxy - sx * sy;
    const double a1 = (double)(2 * sx * sy) + kC1, a2 = (double)(2 * vxy) + kC2;
    const double b1 = (double)(sx * sx + sy * sy) + kC1, b2 = (double)(vxx + vyy) + kC2;
    return (a1 * a2) / (b1 * b2);
}

}  // namespace memc_ssim

#endif  // MEMC_SSIM_MATH_HPP
