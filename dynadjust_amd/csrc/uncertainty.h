// Positional and relative uncertainty of adjusted stations (the quantities of the reference's .apu report, built around the ICSM
// Standard for the Australian Survey Control Network, SP1): a cartesian 3x3 covariance turned into
//   - the local covariance Q = R^T C R, R's columns the east, north and up unit vectors at (lat, lon) in cartesian axes
//     (the rotation of geodesy::LocalToCartRotation), reported as ee en eu nn nu uu;
//   - the 1-sigma horizontal error ellipse: semi-major a, semi-minor b (a^2, b^2 the eigenvalues of the horizontal 2x2 part, b^2
//     clamped at 0), azimuth of the semi-major axis clockwise from north in [0, pi) -- 0 for a circle (a == b to relative 1e-15);
//   - the horizontal PU at 95 %: hz = a (1.960790 + 0.004071 c + 0.114276 c^2 + 0.371625 c^3), c = b / a (0 when a = 0), the SP1
//     approximation of the radius of the circle that holds 95 % of a bivariate normal (within 0.17 % of the exact radius for every
//     c in [0, 1]); the vertical PU at 95 %: vt = 1.96 sqrt(uu).
// PU is defined at 95 % whatever a.confidence_interval is (that setting drives the global test and the outlier flag only).
// One source for the device kernels (uncertainty.hip) and the host debug entry (dnagpu_debug_uncertainty_3x3): every function is
// __host__ __device__.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define UN_HD __host__ __device__ inline
#else
#define UN_HD inline
#endif

namespace dnagpu {
namespace un {

// the fields of dnagpu_uncertainty (include/dnagpu.h), in order
constexpr int RECORD_DOUBLES = 11;
constexpr double PI = 3.14159265358979323846;

// cxyz: xx xy xz yy yz zz; out: enu[6], semi_major, semi_minor, azimuth, hz_pu, vt_pu
UN_HD void uncertainty_3x3(const double* cxyz, double lat, double lon, double* out) {
    const double sl = sin(lat), cl = cos(lat), so = sin(lon), co = cos(lon);
    const double R[3][3] = {{-so, -sl * co, cl * co}, {co, -sl * so, cl * so}, {0.0, cl, sl}};
    const double C[3][3] = {{cxyz[0], cxyz[1], cxyz[2]}, {cxyz[1], cxyz[3], cxyz[4]}, {cxyz[2], cxyz[4], cxyz[5]}};
    double CR[3][3];
    for (int i = 0; i < 3; ++i)
        for (int l = 0; l < 3; ++l) CR[i][l] = C[i][0] * R[0][l] + C[i][1] * R[1][l] + C[i][2] * R[2][l];
    int q = 0;
    for (int k = 0; k < 3; ++k)
        for (int l = k; l < 3; ++l, ++q) out[q] = R[0][k] * CR[0][l] + R[1][k] * CR[1][l] + R[2][k] * CR[2][l];
    const double ee = out[0], en = out[1], nn = out[3], uu = out[5];
    const double mid = 0.5 * (ee + nn), half = 0.5 * (ee - nn);
    const double r = sqrt(half * half + en * en);
    const double a2 = mid + r, b2 = mid - r;
    const double a = a2 > 0.0 ? sqrt(a2) : 0.0, b = b2 > 0.0 ? sqrt(b2) : 0.0;
    double az = 0.0;
    if (a - b > 1e-15 * a) {
        az = 0.5 * atan2(2.0 * en, nn - ee);     // (-pi/2, pi/2]
        if (az < 0.0) az += PI;
        if (az >= PI) az -= PI;
    }
    const double c = a > 0.0 ? b / a : 0.0;
    out[6] = a;
    out[7] = b;
    out[8] = az;
    out[9] = a * (1.960790 + 0.004071 * c + 0.114276 * c * c + 0.371625 * c * c * c);
    out[10] = 1.96 * (uu > 0.0 ? sqrt(uu) : 0.0);
}

// element (r, c) of a symmetric matrix of which only the lower triangle is valid (column-major, leading dimension ld)
UN_HD double lower_sym(const double* S, uint32_t ld, uint32_t r, uint32_t c) {
    return r >= c ? S[(size_t)c * ld + r] : S[(size_t)r * ld + c];
}

// the 3x3 covariance (xx xy xz yy yz zz) of station i, or of the vector from station i to station j:
// D = C_ii + C_jj - C_ij - C_ij^T (i == j: zero)
UN_HD void gather_station(const double* S, uint32_t ld, uint32_t i, double* c6) {
    int q = 0;
    for (int r = 0; r < 3; ++r)
        for (int c = r; c < 3; ++c, ++q) c6[q] = lower_sym(S, ld, 3 * i + r, 3 * i + c);
}
UN_HD void gather_pair(const double* S, uint32_t ld, uint32_t i, uint32_t j, double* c6) {
    int q = 0;
    for (int r = 0; r < 3; ++r)
        for (int c = r; c < 3; ++c, ++q)
            c6[q] = (lower_sym(S, ld, 3 * j + r, 3 * j + c) - lower_sym(S, ld, 3 * i + r, 3 * j + c)) -
                    (lower_sym(S, ld, 3 * j + r, 3 * i + c) - lower_sym(S, ld, 3 * i + r, 3 * i + c));
}

}  // namespace un
}  // namespace dnagpu

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace dnagpu {
// one lane per station / pair; idx: count local station indices (pairs: 2 per pair), latlon: 2 per entry, out: RECORD_DOUBLES per entry
void launch_station_uncertainty(const double* S, uint32_t ld, const uint32_t* idx, const double* latlon, double* out, uint32_t count,
                                hipStream_t st);
void launch_pair_uncertainty(const double* S, uint32_t ld, const uint32_t* idx, const double* latlon, double* out, uint32_t count,
                             hipStream_t st);
}  // namespace dnagpu
#endif
