// fd_kernels_pitch.hip -- F0 tracking by YIN (de Cheveigne and Kawahara 2002) and the pitch scores of a vocoded waveform against its
// recording (include/fastdiff_hip_ext.h: "F0 tracking", which defines the measurement; constants and counts: fd_pitch.h).  The reference
// extracts one F0 per mel frame with Praat / WORLD in its data pipeline (data_gen/tts/data_gen_utils.py: get_pitch); this is YIN on the
// same frame grid.
//
//   k_pitch_track     grid (tiles of PT_FT frames, B).  The samples of the tile's frames are staged in LDS once (consecutive frames
//                     overlap by span - hop; `group` frames at a time where a large hop would not let the whole tile fit).  Then a
//                     wavefront takes one (frame, chunk of 64 lags) after the other, a lane per lag: x[s + j] is an LDS broadcast,
//                     x[s + j + tau] is conflict-free across the lanes.  d(tau) in float32: four accumulators (j mod 4) added as
//                     (a0 + a1) + (a2 + a3), an order that depends on nothing but win.  The sums of the tile go to LDS, then one
//                     wavefront per frame does the rest in float64: the lanes own consecutive runs of lags, the running sum of d is a
//                     scan over the lanes, d' goes to LDS (over the samples, which are no longer needed), k0 (the lowest lag below the
//                     threshold) and k (the lowest lag from k0 on at which the descent stops) are minimum reductions over lag indices,
//                     lane 0 fits the parabola and writes f0 and aper.
//   k_pitch_compare   one workgroup per utterance: counts and the float64 sum of squared cents over 256 consecutive runs of frames,
//                     added in run order -> the 48-byte record.  NaN fields are written as constants chosen from the counts.
//
// Every sum has a fixed order that depends on the utterance alone and there are no atomics, so a row is bit-identical alone, anywhere in
// a ragged batch, at any row pitch and from call to call.  Nothing at or behind an utterance's own length is read.
#include <float.h>
#include <limits.h>
#include <stddef.h>

#include "fd_internal.h"
#include "fd_kernels.h"
#include "fd_kernels_common.h"

namespace fdk {

constexpr int PT_FT = fdp::FRAME_TILE, PT_CHUNK = fdp::LAG_CHUNK;
static_assert(PT_FT == FD_PITCH_FRAME_TILE && PT_CHUNK == FD_PITCH_LAG_CHUNK && fdp::MAX_LAGS == FD_PITCH_MAX_LAGS && fdp::STAGE_FLOATS == FD_PITCH_STAGE_FLOATS, "the exported constants are the kernels'");
static_assert(PT_FT == 4 && PT_CHUNK == 64, "256-thread workgroups: a wavefront per frame in the tail, a lane per lag in the sums");
static_assert(sizeof(fd_pitch) == 48 && sizeof(fd_pitch_config) == 40, "the records of the header");

struct PitchParams { int hop, win, tau_min, tau_max, L, span, group, stage; double rate, threshold; };

__global__ void __launch_bounds__(256) k_pitch_track(const float *__restrict__ x, long long pitch, const long long *__restrict__ lens,
                                                     long long n_all, PitchParams P, float *__restrict__ f0, float *__restrict__ aper,
                                                     long long out_pitch, int F_all)
{
    extern __shared__ double pt_lds[];
    float *xs = reinterpret_cast<float *>(pt_lds);         // [stage]: the samples of a stage group; afterwards 4 x [L] doubles of d'
    float *dsum = xs + P.stage;                            // [PT_FT][L]
    const int b = blockIdx.y, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const long long n = own_len(lens, b, n_all);
    const int F = (int)(n / P.hop);                        // <= F_all
    const int i0 = blockIdx.x * PT_FT;
    const int nf = F - i0 < PT_FT ? (F - i0 > 0 ? F - i0 : 0) : PT_FT;      // frames of this tile that exist
    float *__restrict__ f0_row = f0 + (long long)b * out_pitch, *__restrict__ ap_row = aper + (long long)b * out_pitch;
    if (tid < PT_FT && i0 + tid >= F && i0 + tid < F_all) {      // behind this row's own frames, up to the longest row's
        f0_row[i0 + tid] = 0.0f;
        ap_row[i0 + tid] = 1.0f;
    }
    if (nf == 0) return;                                   // (the whole workgroup)
    const float *__restrict__ row = x + (long long)b * pitch;
    const int nchunk = (P.L + PT_CHUNK - 1) / PT_CHUNK;
    for (int g0 = 0; g0 < nf; g0 += P.group) {
        const int gf = nf - g0 < P.group ? nf - g0 : P.group;
        const long long s0 = (long long)(i0 + g0) * P.hop + P.hop / 2 - P.span / 2;
        const int cnt = P.span + (gf - 1) * P.hop;         // <= stage (fdp::stage_floats)
        __syncthreads();
        for (int t = tid; t < cnt; t += 256) {
            const long long p = s0 + t;
            xs[t] = p >= 0 && p < n ? row[p] : 0.0f;
        }
        __syncthreads();
        for (int item = wv; item < gf * nchunk; item += 4) {
            const int f = item / nchunk, tau = (item - f * nchunk) * PT_CHUNK + lane;
            if (tau >= P.L) continue;
            const float *a = xs + f * P.hop, *c = a + tau;      // c[j] for j < win: at most f hop + win - 1 + tau_max + 1 = f hop + span - 1 < cnt
            float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
            int j = 0;
            for (; j + 4 <= P.win; j += 4) {
                const float e0 = a[j] - c[j], e1 = a[j + 1] - c[j + 1], e2 = a[j + 2] - c[j + 2], e3 = a[j + 3] - c[j + 3];
                a0 = fmaf(e0, e0, a0); a1 = fmaf(e1, e1, a1); a2 = fmaf(e2, e2, a2); a3 = fmaf(e3, e3, a3);
            }
            if (j < P.win) { const float e = a[j] - c[j]; a0 = fmaf(e, e, a0); ++j; }
            if (j < P.win) { const float e = a[j] - c[j]; a1 = fmaf(e, e, a1); ++j; }
            if (j < P.win) { const float e = a[j] - c[j]; a2 = fmaf(e, e, a2); }
            dsum[(g0 + f) * P.L + tau] = __fadd_rn(__fadd_rn(a0, a1), __fadd_rn(a2, a3));
        }
    }
    __syncthreads();                                       // the sums are complete and nobody reads the samples any more

    // steps 3-5 in float64, wavefront wv on frame i0 + wv; lane l owns the lags [l R, l R + R)
    const bool live = wv < nf;
    const int R = (P.L + 63) / 64;
    const int t0 = lane * R, t1 = t0 + R < P.L ? t0 + R : P.L;
    const float *d = dsum + wv * P.L;
    double *dp = pt_lds + wv * P.L;
    if (live) {
        double local = 0.0;
        for (int t = t0 > 1 ? t0 : 1; t < t1; ++t) local += (double)d[t];
        double incl = local;
        for (int off = 1; off < 64; off <<= 1) {
            const double v = __shfl_up(incl, off, 64);
            if (lane >= off) incl += v;
        }
        double run = __shfl_up(incl, 1, 64);               // the sum of d(1 ..) over the lanes before this one
        if (lane == 0) run = 0.0;
        for (int t = t0; t < t1; ++t) {
            if (t == 0) { dp[0] = 1.0; continue; }
            const double v = (double)d[t];
            run += v;
            dp[t] = run > 0.0 ? v * (double)t / run : 1.0;
        }
    }
    __syncthreads();
    if (!live) return;
    int k0 = INT_MAX;
    double mn = DBL_MAX;
    for (int t = t0; t < t1; ++t) {
        if (t < P.tau_min || t > P.tau_max) continue;
        const double v = dp[t];
        mn = v < mn ? v : mn;
        if (v < P.threshold && k0 == INT_MAX) k0 = t;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_xor(k0, off, 64);
        const double m = __shfl_xor(mn, off, 64);
        k0 = o < k0 ? o : k0;
        mn = m < mn ? m : mn;
    }
    const int i = i0 + wv;
    if (k0 == INT_MAX) {                                   // (the whole wavefront) unvoiced
        if (lane == 0) { f0_row[i] = 0.0f; ap_row[i] = (float)mn; }
        return;
    }
    int k = INT_MAX;                                       // the lowest t >= k0 at which the descent stops; t = tau_max always does
    for (int t = t0; t < t1 && k == INT_MAX; ++t) {
        if (t < k0 || t > P.tau_max) continue;
        if (!(t + 1 <= P.tau_max && dp[t + 1] < dp[t])) k = t;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_xor(k, off, 64);
        k = o < k ? o : k;
    }
    if (lane == 0) {                                       // 2 <= tau_min <= k <= tau_max = L - 2
        const double pa = dp[k - 1], pb = dp[k], pc = dp[k + 1];
        const double den = pa - 2.0 * pb + pc;
        double off = den > 0.0 ? 0.5 * (pa - pc) / den : 0.0;
        off = off < -1.0 ? -1.0 : (off > 1.0 ? 1.0 : off);
        f0_row[i] = (float)(P.rate / ((double)k + off));
        ap_row[i] = (float)pb;
    }
}

__global__ void __launch_bounds__(256) k_pitch_compare(const float *__restrict__ fr, const float *__restrict__ fd, long long pitch,
                                                       const long long *__restrict__ frames, long long F_all, fd_pitch *__restrict__ rec)
{
    __shared__ double ssum[256];
    __shared__ int scnt[256][5];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int F = (int)own_len(frames, b, F_all);
    const float *__restrict__ r = fr + (long long)b * pitch, *__restrict__ g = fd + (long long)b * pitch;
    const int run = (F + 255) / 256;
    double sum = 0.0;
    int both = 0, nr = 0, nd = 0, differ = 0, gross = 0;
    for (long long i = (long long)tid * run; i < F && i < (long long)(tid + 1) * run; ++i) {
        const float a = r[i], c = g[i];
        const bool va = a > 0.0f, vc = c > 0.0f;
        nr += va; nd += vc; differ += va != vc;
        if (va && vc) {
            const double ratio = (double)c / (double)a;
            const double cents = 1200.0 * log2(ratio);
            sum += cents * cents;
            gross += fabs(ratio - 1.0) > 0.2;
            ++both;
        }
    }
    ssum[tid] = sum;
    scnt[tid][0] = both; scnt[tid][1] = nr; scnt[tid][2] = nd; scnt[tid][3] = differ; scnt[tid][4] = gross;
    __syncthreads();
    if (tid != 0) return;
    sum = 0.0; both = nr = nd = differ = gross = 0;
    for (int t = 0; t < 256; ++t) {
        sum += ssum[t];
        both += scnt[t][0]; nr += scnt[t][1]; nd += scnt[t][2]; differ += scnt[t][3]; gross += scnt[t][4];
    }
    // the three doubles go out as 64-bit integers: the NaN of a field that does not apply is a bit pattern chosen from the counts, which
    // no reading of -fno-honor-nans can turn into something else
    const long long nan_bits = __double_as_longlong(quiet_nan());
    const int status = F == 0 ? FD_PITCH_SHORT : (both == 0 ? FD_PITCH_UNVOICED : FD_PITCH_OK);
    long long rmse_bits = nan_bits, gpe_bits = nan_bits, vde_bits = nan_bits;
    if (status == FD_PITCH_OK) {
        rmse_bits = __double_as_longlong(sqrt(sum / (double)both));
        gpe_bits = __double_as_longlong((double)gross / (double)both);
    }
    if (status != FD_PITCH_SHORT) vde_bits = __double_as_longlong((double)differ / (double)F);
    static_assert(offsetof(fd_pitch, rmse_cents) == 0 && offsetof(fd_pitch, gpe) == 8 && offsetof(fd_pitch, vde) == 16 && offsetof(fd_pitch, frames) == 24,
                  "three doubles, then six int32");
    long long *words = reinterpret_cast<long long *>(rec + b);
    int *ints = reinterpret_cast<int *>(words + 3);
    words[0] = rmse_bits; words[1] = gpe_bits; words[2] = vde_bits;
    ints[0] = F; ints[1] = both; ints[2] = nr; ints[3] = nd; ints[4] = status; ints[5] = 0;
}

hipError_t pitch_track(const Launch &La, const float *wav, long long pitch, int B, int64_t L, const long long *lens_dev,
                       const fd_pitch_config &cfg, const fdp::Lags &lg, float *f0, float *aper, long long out_pitch)
{
    const int64_t F_all = fdp::frames(L, cfg.hop);
    if (F_all == 0) return hipSuccess;
    PitchParams P;
    P.hop = cfg.hop; P.win = cfg.win; P.tau_min = lg.tau_min; P.tau_max = lg.tau_max; P.L = lg.L; P.span = lg.span;
    P.group = fdp::stage_group(lg.span, cfg.hop);
    P.stage = fdp::stage_floats(lg.span, cfg.hop, lg.L);
    P.rate = (double)cfg.rate; P.threshold = cfg.threshold;
    FD_LAUNCH(La, "pitch_track", k_pitch_track, dim3((unsigned)((F_all + PT_FT - 1) / PT_FT), B), dim3(256), fdp::lds_bytes(lg.span, cfg.hop, lg.L),
              wav, pitch, lens_dev, (long long)L, P, f0, aper, out_pitch, (int)F_all);
    return hipSuccess;
}

hipError_t pitch_compare(const Launch &La, const float *f0_ref, const float *f0_deg, long long pitch, int B, const long long *frames_dev,
                         fd_pitch *rec)
{
    FD_LAUNCH(La, "pitch_compare", k_pitch_compare, dim3(B), dim3(256), 0, f0_ref, f0_deg, pitch, frames_dev, pitch, rec);
    return hipSuccess;
}

}  // namespace fdk
