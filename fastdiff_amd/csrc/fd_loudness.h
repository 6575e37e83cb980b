// fd_loudness.h -- host side of the loudness meter (include/fastdiff_hip_ext.h: "BS.1770 loudness"): the K-weighting design, the block
// count, and the cascade as a 4-state linear system with the powers of its matrix that the kernels combine run and tile states with.
// Plain C++ without the HIP runtime, so a stand-alone host program can include it.  tests/loudness_ref.py is the float64 oracle.
#pragma once
#include <math.h>
#include <stdint.h>

namespace fdl {

constexpr int RATE_MIN = 8000, RATE_MAX = 192000;
constexpr int RUN = 64, LANES = 256, TILE = RUN * LANES;      // FD_LOUDNESS_TILE
constexpr int POWERS = 9;                                     // A^(RUN << k), k = 0 .. 8; the last is A^TILE
constexpr double T_G = 0.4, STEP = 0.25;

// What the kernels receive by value: c = shelf b0 b1 b2 a1 a2, high pass b0 b1 b2 a1 a2; P[k] = A^(RUN << k), row-major 4 x 4.
struct Filter {
    double c[10];
    double P[POWERS][16];
};

inline bool rate_ok(int rate) { return rate >= RATE_MIN && rate <= RATE_MAX; }

inline void design(int rate, double *c)
{
    const double pi = 3.14159265358979323846;
    {   // high shelf: G = 4 dB, Q = 1 / sqrt 2, fc = 1500
        const double A = pow(10.0, 4.0 / 40.0), w0 = 2.0 * pi * (1500.0 / rate), alpha = sin(w0) / (2.0 * (1.0 / sqrt(2.0)));
        const double co = cos(w0), s = 2.0 * sqrt(A) * alpha;
        const double b0 = A * ((A + 1) + (A - 1) * co + s), b1 = -2 * A * ((A - 1) + (A + 1) * co), b2 = A * ((A + 1) + (A - 1) * co - s);
        const double a0 = (A + 1) - (A - 1) * co + s, a1 = 2 * ((A - 1) - (A + 1) * co), a2 = (A + 1) - (A - 1) * co - s;
        c[0] = b0 / a0; c[1] = b1 / a0; c[2] = b2 / a0; c[3] = a1 / a0; c[4] = a2 / a0;
    }
    {   // high pass: Q = 0.5, fc = 38
        const double w0 = 2.0 * pi * (38.0 / rate), alpha = sin(w0) / (2.0 * 0.5), co = cos(w0);
        const double b0 = (1 + co) / 2, b1 = -(1 + co), b2 = (1 + co) / 2, a0 = 1 + alpha, a1 = -2 * co, a2 = 1 - alpha;
        c[5] = b0 / a0; c[6] = b1 / a0; c[7] = b2 / a0; c[8] = a1 / a0; c[9] = a2 / a0;
    }
}

// nb = int(round((n / rate - T_g) / (T_g step)) + 1), round half to even (the default rounding mode's rint); 0: shorter than one block
inline int64_t blocks(int64_t n, int rate)
{
    if (n < (int64_t)(T_G * rate)) return 0;
    const double T = (double)n / (double)rate;
    return (int64_t)(rint((T - T_G) / (T_G * STEP)) + 1);
}

inline void matmul4(const double *a, const double *b, double *out)
{
    double r[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += a[i * 4 + k] * b[k * 4 + j];
            r[i * 4 + j] = s;
        }
    for (int i = 0; i < 16; ++i) out[i] = r[i];
}

// Both biquads in transposed direct form II, states (s1, s2, t1, t2):
//   y1 = b0 x + s1,  s1' = b1 x - a1 y1 + s2,  s2' = b2 x - a2 y1;   y2 = c0 y1 + t1,  t1' = c1 y1 - d1 y2 + t2,  t2' = c2 y1 - d2 y2
// so with x = 0:  s1' = -a1 s1 + s2,  s2' = -a2 s1,  t1' = (c1 - d1 c0) s1 - d1 t1 + t2,  t2' = (c2 - d2 c0) s1 - d2 t1.
inline void make_filter(int rate, Filter &F)
{
    design(rate, F.c);
    const double *c = F.c;
    const double A[16] = {-c[3], 1, 0, 0,
                          -c[4], 0, 0, 0,
                          c[6] - c[8] * c[5], 0, -c[8], 1,
                          c[7] - c[9] * c[5], 0, -c[9], 0};
    double M[16];
    for (int i = 0; i < 16; ++i) M[i] = A[i];
    for (int r = 1; r < RUN; r <<= 1) matmul4(M, M, M);      // A^RUN (RUN is a power of two)
    static_assert((RUN & (RUN - 1)) == 0, "A^RUN by squaring");
    for (int k = 0; k < POWERS; ++k) {
        for (int i = 0; i < 16; ++i) F.P[k][i] = M[i];
        matmul4(M, M, M);
    }
}

}  // namespace fdl
