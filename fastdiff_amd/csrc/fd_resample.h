// fd_resample.h -- host side of the resampler's filter design (include/fastdiff_hip_ext.h: "Sample-rate conversion"): the reduced ratio,
// the output length, the Kaiser-windowed sinc prototype in double and the polyphase table the kernel reads.  Plain C++ without the HIP
// runtime, so a stand-alone host program can include it.  fastdiff_amd/resample.py: design() is its numpy twin.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

namespace fdr {

constexpr int ZEROS = 64;                              // zero crossings per side at the narrower rate
constexpr double ROLLOFF = 0.9475937167399596;         // cut-off as a fraction of the narrower Nyquist
constexpr double BETA = 14.769656459379492;            // Kaiser window shape
constexpr int MAX_RATIO = 1024;                        // FD_RESAMPLE_MAX_RATIO

struct Ratio { int up, down, half, K, Kp; };           // K taps per output, Kp = K rounded up to 4

// false: a rate < 1.  The ratio may still be too wide (max(up, down) > MAX_RATIO): the callers refuse that.
inline bool reduce(int sr_in, int sr_out, Ratio &r)
{
    if (sr_in < 1 || sr_out < 1) return false;
    int a = sr_in, b = sr_out;
    while (b) { const int t = a % b; a = b; b = t; }
    r.up = sr_out / a;
    r.down = sr_in / a;
    const int q = r.up > r.down ? r.up : r.down;
    r.half = q <= MAX_RATIO ? ZEROS * q : 0;
    r.K = q <= MAX_RATIO ? (2 * r.half + 1 + r.up - 1) / r.up : 0;
    r.Kp = (r.K + 3) & ~3;
    return true;
}

// ceil(n up / down) without overflow for any n >= 0 that fits int64 together with its result (n / down * up + ...: up, down <= 2^31)
inline int64_t out_len(int64_t n, const Ratio &r)
{
    const int64_t whole = n / r.down, rest = n % r.down;      // n up / down = whole up + rest up / down, rest up < 2^62
    return whole * r.up + (rest * r.up + r.down - 1) / r.down;
}

// Modified Bessel function of the first kind, order 0: sum_k ((x/2)^k / k!)^2.  All terms positive, so the sum is accurate to a few ulp;
// for x <= 15 the terms fall under 1e-17 of the sum within 40 of them.
inline double bessel_i0(double x)
{
    const double y = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= y / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

// g[0 .. 2 half]: sinc(rolloff (k - half) / q) kaiser(k; 2 half + 1, beta), divided by its sum
inline std::vector<double> prototype(const Ratio &r)
{
    const double pi = 3.14159265358979323846;
    const int half = r.half, n = 2 * half + 1, q = r.up > r.down ? r.up : r.down;
    std::vector<double> g(n);
    const double i0b = bessel_i0(BETA);
    double sum = 0.0;
    for (int k = 0; k < n; ++k) {
        const double m = (double)(k - half), t = ROLLOFF * m / q;
        const double s = k == half ? 1.0 : sin(pi * t) / (pi * t);
        const double u = m / half;                              // -1 .. 1 (half >= 64)
        const double w = bessel_i0(BETA * sqrt(1.0 - u * u > 0.0 ? 1.0 - u * u : 0.0)) / i0b;
        g[k] = s * w;
        sum += g[k];
    }
    for (int k = 0; k < n; ++k) g[k] /= sum;
    return g;
}

// h = up g, rounded once to float32
inline std::vector<float> taps(const Ratio &r)
{
    const std::vector<double> g = prototype(r);
    std::vector<float> h(g.size());
    for (size_t k = 0; k < g.size(); ++k) h[k] = (float)((double)r.up * g[k]);
    return h;
}

// The kernel's table [up][Kp].  Output i has a = i down + half, phase p = a % up and last input jmax = a / up; its products are
// x[jmax - m] h[p + m up], m = 0 .. K - 1.  Row p holds them in the order of ascending input: table[p][r] = h[p + (K - 1 - r) up]
// (0 where that index passes 2 half, and in the padding r >= K), to be multiplied with x[jmax - (K - 1) + r].
inline std::vector<float> table(const Ratio &r)
{
    const std::vector<float> h = taps(r);
    std::vector<float> t((size_t)r.up * r.Kp, 0.0f);
    for (int p = 0; p < r.up; ++p)
        for (int k = 0; k < r.K; ++k) {
            const int64_t idx = (int64_t)p + (int64_t)(r.K - 1 - k) * r.up;
            if (idx <= 2 * (int64_t)r.half) t[(size_t)p * r.Kp + k] = h[idx];
        }
    return t;
}

}  // namespace fdr
