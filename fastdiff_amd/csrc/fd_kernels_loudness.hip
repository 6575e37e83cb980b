// fd_kernels_loudness.hip -- BS.1770 loudness on the device (include/fastdiff_hip_ext.h: fd_loudness_measure / fd_loudness_normalize):
// what the reference gets from pyloudnorm.Meter(rate).integrated_loudness and pyln.normalize.loudness in process_utterance(loud_norm=True)
// (data_gen/tts/data_gen_utils.py:115-120), and the level control behind the vocoder next to wav / abs(wav).max().
//
// The K-weighting cascade is a linear recurrence s' = A s + B x over 4 float64 states (csrc/fd_loudness.h).  It is computed exactly:
//
//   k_loud_pass<false>   grid (tiles, B).  A workgroup stages its tile of LD_TILE samples through LDS into registers, LD_RUN = 64
//                        consecutive samples per lane; every lane runs its samples from zero state; an inclusive scan over the 256 lanes
//                        (step k: e[i] = A^(64 << k) e[i - (1 << k)] + e[i]) leaves the tile's zero-state end state in the last lane.
//                        Also the utterance's peak (atomicMax on non-negative float bits: no order to depend on).
//   k_loud_carry         one workgroup per utterance: S[t + 1] = A^TILE S[t] + E[t], in place, tile states staged through LDS.
//   k_loud_pass<true>    the same staging; lane 0 starts from the tile's true state, the scan then gives every lane its true incoming
//                        state; the run is done again from it and y^2 summed per 100 ms segment: a lane adds its samples in ascending
//                        order (two partials if its run straddles a segment border -- a segment is at least 799 samples), the tile's
//                        partials are added per segment over lanes in a fixed order (8 groups of 32 lanes, each in lane order, then
//                        the 8 sums in group order).
//   k_loud_gate          one workgroup per utterance: segment sums over tiles in tile order, block powers (4 consecutive segments),
//                        both gates, LUFS, gain and status -> the 32-byte record.
//   k_loud_apply         wav gain -> float32 / int16, or the peak epilogue's arithmetic for SHORT / SILENT / CLIPPED utterances.
//
// The filtered signal never reaches memory.  Samples at or behind an utterance's own length are never loaded (x = 0 in their place and
// nothing of them is summed), so an utterance's numbers are the same alone and in a ragged batch.
#include "fd_internal.h"
#include "fd_kernels.h"
#include "fd_kernels_common.h"

namespace fdk {

constexpr int LD_RUN = fdl::RUN, LD_LANES = fdl::LANES, LD_TILE = fdl::TILE, LD_SEGS = LOUDNESS_SEGS;
static_assert(LD_TILE == FD_LOUDNESS_TILE && LD_LANES == 256 && LD_RUN == 64, "a tile is 256 lanes x 64 samples");
constexpr int LD_HALF = LD_TILE / 2, LD_PITCH = LD_RUN + 1;      // staged half a tile at a time, rows padded against bank conflicts

struct LdState { double s1, s2, t1, t2; };

// one sample through both biquads (transposed direct form II); returns the K-weighted sample
__device__ __forceinline__ double ld_step(const double *__restrict__ c, LdState &s, double x)
{
    const double y1 = c[0] * x + s.s1;
    s.s1 = c[1] * x - c[3] * y1 + s.s2;
    s.s2 = c[2] * x - c[4] * y1;
    const double y2 = c[5] * y1 + s.t1;
    s.t1 = c[6] * y1 - c[8] * y2 + s.t2;
    s.t2 = c[7] * y1 - c[9] * y2;
    return y2;
}

__device__ __forceinline__ LdState ld_matvec_add(const double *__restrict__ M, const LdState &v, const LdState &e)
{
    LdState r;      // two halves per row: a dependent chain of three operations instead of five (the carry kernel is one such chain per tile)
    r.s1 = (M[0] * v.s1 + M[1] * v.s2) + (M[2] * v.t1 + (M[3] * v.t2 + e.s1));
    r.s2 = (M[4] * v.s1 + M[5] * v.s2) + (M[6] * v.t1 + (M[7] * v.t2 + e.s2));
    r.t1 = (M[8] * v.s1 + M[9] * v.s2) + (M[10] * v.t1 + (M[11] * v.t2 + e.t1));
    r.t2 = (M[12] * v.s1 + M[13] * v.s2) + (M[14] * v.t1 + (M[15] * v.t2 + e.t2));
    return r;
}

// first sample of 100 ms segment j: int(T_g (j step) rate) in double, in this order (block j = segments j .. j + 3)
__device__ __forceinline__ long long ld_seg_lo(long long j, double rate) { return (long long)((0.4 * ((double)j * 0.25)) * rate); }
// the segment that holds sample i
__device__ __forceinline__ long long ld_seg_of(long long i, double rate)
{
    long long j = (long long)((double)i / (0.1 * rate));
    while (j > 0 && ld_seg_lo(j, rate) > i) --j;
    while (ld_seg_lo(j + 1, rate) <= i) ++j;
    return j;
}

// inclusive scan of the lanes' end states: afterwards lane i holds the end state of lanes 0 .. i run one after the other
__device__ __forceinline__ LdState ld_scan(const LoudnessFilter &F, LdState e, double *sc, int tid)
{
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int off = 1 << k;
        __syncthreads();
        sc[tid] = e.s1; sc[256 + tid] = e.s2; sc[512 + tid] = e.t1; sc[768 + tid] = e.t2;
        __syncthreads();
        if (tid >= off) {
            LdState p;
            p.s1 = sc[tid - off]; p.s2 = sc[256 + tid - off]; p.t1 = sc[512 + tid - off]; p.t2 = sc[768 + tid - off];
            e = ld_matvec_add(F.P[k], p, e);
        }
    }
    return e;
}

template <bool SUMS>
__global__ void __launch_bounds__(256) k_loud_pass(const float *__restrict__ wav, long long L, const long long *__restrict__ valid, int tiles,
                                                   double *__restrict__ state, double *__restrict__ part, unsigned int *__restrict__ peakbits,
                                                   double rate, LoudnessFilter F)
{
    __shared__ float xs[(LD_LANES / 2) * LD_PITCH];
    __shared__ double sc[4 * LD_LANES];
    __shared__ int sq[LD_LANES];
    __shared__ float wm[4];
    const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
    const long long n = own_len(valid, b, L);
    const long long t0 = (long long)t * LD_TILE;
    if (t0 >= n) return;                                   // (the whole workgroup) a tile behind the utterance: nothing reads its slots
    const float *__restrict__ row = wav + (long long)b * L;
    float x[LD_RUN];
    float m = 0.0f;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        __syncthreads();
        for (int k = 0; k < LD_HALF / 256; ++k) {
            const int il = k * 256 + tid;
            const long long gi = t0 + c * LD_HALF + il;
            const float v = gi < n ? row[gi] : 0.0f;
            m = fmaxf(m, fabsf(v));
            xs[(il >> 6) * LD_PITCH + (il & 63)] = v;
        }
        __syncthreads();
        if ((tid >> 7) == c) {
#pragma unroll
            for (int k = 0; k < LD_RUN; ++k) x[k] = xs[(tid & 127) * LD_PITCH + k];
        }
    }
    if (!SUMS) {
        for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_down(m, off, 64));
        if ((tid & 63) == 0) wm[tid >> 6] = m;
        __syncthreads();
        if (tid == 0) atomicMax(peakbits + b, __float_as_uint(fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]))));
    }
    double *st = state + ((long long)b * tiles + t) * 4;
    LdState s = {0.0, 0.0, 0.0, 0.0};
    if (SUMS && tid == 0) { s.s1 = st[0]; s.s2 = st[1]; s.t1 = st[2]; s.t2 = st[3]; }
    const LdState s_in = s;
#pragma unroll
    for (int k = 0; k < LD_RUN; ++k) (void)ld_step(F.c, s, (double)x[k]);
    s = ld_scan(F, s, sc, tid);
    if (!SUMS) {
        if (tid == LD_LANES - 1) { st[0] = s.s1; st[1] = s.s2; st[2] = s.t1; st[3] = s.t2; }
        return;
    }
    // the true incoming state of every lane: the end state of the lanes before it
    __syncthreads();
    sc[tid] = s.s1; sc[256 + tid] = s.s2; sc[512 + tid] = s.t1; sc[768 + tid] = s.t2;
    __syncthreads();
    s = s_in;
    if (tid > 0) { s.s1 = sc[tid - 1]; s.s2 = sc[256 + tid - 1]; s.t1 = sc[512 + tid - 1]; s.t2 = sc[768 + tid - 1]; }
    // this lane's samples [start, start + cnt), the first kb of them in segment q0 (tile-local), the others in q0 + 1
    const long long start = t0 + (long long)tid * LD_RUN;
    const int cnt = n - start >= LD_RUN ? LD_RUN : (n > start ? (int)(n - start) : 0);
    const long long seg_first = ld_seg_of(t0, rate);
    int q0 = -2, kb = 0;
    if (cnt > 0) {
        const long long s0 = ld_seg_of(start, rate), border = ld_seg_lo(s0 + 1, rate) - start;
        q0 = (int)(s0 - seg_first);
        kb = border < cnt ? (int)border : cnt;
    }
    double p0 = 0.0, p1 = 0.0;
#pragma unroll
    for (int k = 0; k < LD_RUN; ++k) {
        const double y = ld_step(F.c, s, (double)x[k]);
        const double y2 = y * y;
        p0 += k < kb ? y2 : 0.0;
        p1 += (k >= kb && k < cnt) ? y2 : 0.0;
    }
    __syncthreads();
    sc[tid] = p0; sc[256 + tid] = p1; sq[tid] = q0;
    __syncthreads();
    // per segment: 8 threads add the partials of 32 lanes each in lane order, then one adds the 8 sums in that order
    const int q = tid >> 3, g = tid & 7;
    if (q < LD_SEGS) {
        double sum = 0.0;
        for (int l = g * 32; l < g * 32 + 32; ++l) {
            const int ql = sq[l];
            sum += ql == q ? sc[l] : 0.0;
            sum += ql + 1 == q ? sc[256 + l] : 0.0;
        }
        sc[512 + tid] = sum;
    }
    __syncthreads();
    if (q < LD_SEGS && g == 0) {
        double sum = sc[512 + tid];
        for (int k = 1; k < 8; ++k) sum += sc[512 + tid + k];
        part[((long long)b * tiles + t) * LD_SEGS + q] = sum;
    }
}

__global__ void __launch_bounds__(64) k_loud_carry(double *__restrict__ state, long long L, const long long *__restrict__ valid, int tiles,
                                                   LoudnessFilter F)
{
    __shared__ double buf[4 * 256], outb[4 * 256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const long long n = own_len(valid, b, L);
    const int nt = (int)((n + LD_TILE - 1) / LD_TILE);
    double *st = state + (long long)b * tiles * 4;
    LdState cur = {0.0, 0.0, 0.0, 0.0};
    for (int c0 = 0; c0 < nt; c0 += 256) {
        const int mcnt = nt - c0 < 256 ? nt - c0 : 256;
        for (int i = tid; i < mcnt * 4; i += 64) buf[i] = st[(long long)c0 * 4 + i];
        __syncthreads();
        if (tid == 0) {      // reads and writes in different arrays, so the reads of the next tiles do not wait for this one's chain
            const double *__restrict__ in = buf;
            double *__restrict__ out = outb;
#pragma unroll 8
            for (int k = 0; k < mcnt; ++k) {
                const LdState e = {in[k * 4], in[k * 4 + 1], in[k * 4 + 2], in[k * 4 + 3]};
                out[k * 4] = cur.s1; out[k * 4 + 1] = cur.s2; out[k * 4 + 2] = cur.t1; out[k * 4 + 3] = cur.t2;
                cur = ld_matvec_add(F.P[fdl::POWERS - 1], cur, e);
            }
        }
        __syncthreads();
        for (int i = tid; i < mcnt * 4; i += 64) st[(long long)c0 * 4 + i] = outb[i];
        __syncthreads();
    }
}

// sum of two (count, sum) pairs per thread over the workgroup, in a fixed tree; every thread gets the result
__device__ __forceinline__ void ld_block_sum(double *sc, int tid, double &cnt, double &sum)
{
    __syncthreads();
    sc[tid] = cnt; sc[256 + tid] = sum;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) { sc[tid] += sc[tid + off]; sc[256 + tid] += sc[256 + tid + off]; }
        __syncthreads();
    }
    cnt = sc[0]; sum = sc[256];
}

__global__ void __launch_bounds__(256) k_loud_gate(long long L, const long long *__restrict__ valid, int tiles, const double *__restrict__ part,
                                                   const unsigned int *__restrict__ peakbits, double *__restrict__ zbuf, long long zpitch,
                                                   long long zoff, double rate, int normalize, double target, fd_loudness *__restrict__ rec)
{
    __shared__ double sc[512];
    const int b = blockIdx.x, tid = threadIdx.x;
    const long long n = own_len(valid, b, L);
    const float peak = __uint_as_float(peakbits[b]);
    fd_loudness r;
    r.lufs = -__builtin_huge_val(); r.gain = 1.0f; r.peak = peak; r.blocks = 0; r.gated = 0; r.status = FD_LOUDNESS_SHORT; r.reserved = 0;
    if (n < (long long)(0.4 * rate)) {
        if (tid == 0) rec[b] = r;
        return;
    }
    const double T = (double)n / rate;
    const long long nb = (long long)(__builtin_rint((T - 0.4) / (0.4 * 0.25)) + 1.0);
    const double div = 0.4 * rate;
    const double *pt = part + (long long)b * tiles * LD_SEGS;
    double *seg = zbuf + (long long)b * zpitch, *z = seg + zoff;
    for (long long s = tid; s < nb + 3; s += 256) {        // every segment summed over its tiles in tile order
        const long long lo = ld_seg_lo(s, rate);
        long long hi = ld_seg_lo(s + 1, rate);
        hi = hi < n ? hi : n;
        double ss = 0.0;
        if (lo < hi)
            for (long long t = lo / LD_TILE; t <= (hi - 1) / LD_TILE; ++t) {
                const long long q = s - ld_seg_of(t * LD_TILE, rate);      // 0 .. 22 at 8000 Hz and above
                if (q >= 0 && q < LD_SEGS) ss += pt[t * LD_SEGS + q];
            }
        seg[s] = ss;
    }
    __syncthreads();
    double cj = 0.0, sj = 0.0;
    for (long long j = tid; j < nb; j += 256) {            // block j = segments j .. j + 3
        const double zj = (((seg[j] + seg[j + 1]) + seg[j + 2]) + seg[j + 3]) / div;
        z[j] = zj;
        const double lj = -0.691 + 10.0 * log10(zj);       // z = 0: -inf, which passes no gate
        if (lj >= -70.0) { cj += 1.0; sj += zj; }
    }
    ld_block_sum(sc, tid, cj, sj);
    r.blocks = (int)nb;
    r.status = FD_LOUDNESS_SILENT;
    if (cj == 0.0) {
        if (tid == 0) rec[b] = r;
        return;
    }
    const double gamma = -0.691 + 10.0 * log10(sj / cj) - 10.0;
    double cg = 0.0, sg = 0.0;
    for (long long j = tid; j < nb; j += 256) {             // the z this thread wrote itself
        const double zj = z[j];
        const double lj = -0.691 + 10.0 * log10(zj);
        if (lj > gamma && lj > -70.0) { cg += 1.0; sg += zj; }
    }
    ld_block_sum(sc, tid, cg, sg);
    if (tid != 0) return;
    if (cg > 0.0) {
        r.gated = (int)cg;
        r.lufs = -0.691 + 10.0 * log10(sg / cg);
        r.status = FD_LOUDNESS_OK;
        if (normalize) {
            const double g = pow(10.0, (target - r.lufs) / 20.0);
            if ((double)peak * g > 1.0) {
                r.status = FD_LOUDNESS_CLIPPED;
                r.gain = 1.0f / peak;
            } else {
                r.gain = (float)g;
            }
        }
    }
    rec[b] = r;
}

template <typename OUT>
__global__ void k_loud_apply(const float *__restrict__ wav, long long L, const long long *__restrict__ valid, const fd_loudness *__restrict__ rec,
                             OUT *__restrict__ out)
{
    constexpr bool PCM = sizeof(OUT) == 2;
    const int b = blockIdx.y;
    const long long n = own_len(valid, b, L);
    const int status = rec[b].status;
    const float gain = rec[b].gain, m = rec[b].peak;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < L; i += (long long)gridDim.x * blockDim.x) {
        const float w = wav[(long long)b * L + i];
        if (PCM) {
            // SHORT, SILENT and CLIPPED: the peak epilogue's own arithmetic (k_to_int16)
            const float v = status == FD_LOUDNESS_OK ? w * gain : w / m;
            out[(long long)b * L + i] = i < n ? (OUT)(v * 32767.0f) : (OUT)0;
        } else {
            const float v = status == FD_LOUDNESS_OK ? w * gain : (status == FD_LOUDNESS_CLIPPED ? w / m : w);
            out[(long long)b * L + i] = i < n ? (OUT)v : (OUT)0;
        }
    }
}

// the scratch buffer: peak words [B], valid [B], records [B], tile states [B][tiles][4], partials [B][tiles][LD_SEGS], segment sums and block powers [B][zpitch]
struct LdLayout { size_t peak, valid, rec, state, part, z, total; int tiles; long long zpitch, zoff; };
static LdLayout ld_layout(int B, int64_t L, int rate)
{
    LdLayout o;
    o.tiles = (int)((L + LD_TILE - 1) / LD_TILE);
    const int64_t nb = fdl::blocks(L, rate);
    o.zoff = nb + 4;                                       // per utterance: segment sums [nb + 3], then block powers [nb]
    o.zpitch = o.zoff + nb + 4;
    Carve c;
    o.peak = c.take(sizeof(unsigned int) * B);
    o.valid = c.take(sizeof(long long) * B);
    o.rec = c.take(sizeof(fd_loudness) * B);
    o.state = c.take(sizeof(double) * 4 * (size_t)B * o.tiles);
    o.part = c.take(sizeof(double) * LD_SEGS * (size_t)B * o.tiles);
    o.z = c.take(sizeof(double) * (size_t)B * (size_t)o.zpitch);
    o.total = c.at;
    return o;
}

size_t loudness_scratch_bytes(int B, int64_t L, int rate) { return ld_layout(B, L, rate).total; }
long long *loudness_valid_slot(void *scratch, int B, int64_t L, int rate) { return reinterpret_cast<long long *>(static_cast<char *>(scratch) + ld_layout(B, L, rate).valid); }

hipError_t loudness(const Launch &La, const float *wav, int B, int64_t L, const long long *valid_dev, int rate, const LoudnessFilter &F,
                    bool normalize, double target, fd_loudness *rec, float *out_f32, int16_t *out_pcm, void *scratch)
{
    const LdLayout o = ld_layout(B, L, rate);
    char *base = static_cast<char *>(scratch);
    unsigned int *peakbits = reinterpret_cast<unsigned int *>(base + o.peak);
    double *state = reinterpret_cast<double *>(base + o.state), *part = reinterpret_cast<double *>(base + o.part);
    double *z = reinterpret_cast<double *>(base + o.z);
    if (!rec) rec = reinterpret_cast<fd_loudness *>(base + o.rec);
    hipError_t e = hipMemsetAsync(peakbits, 0, sizeof(unsigned int) * B, La.stream);
    if (e != hipSuccess) return e;
    const dim3 grid(o.tiles, B);
    FD_LAUNCH(La, "loudness_pass1", k_loud_pass<false>, grid, dim3(256), 0, wav, (long long)L, valid_dev, o.tiles, state, part, peakbits,
              (double)rate, F);
    FD_LAUNCH(La, "loudness_carry", k_loud_carry, dim3(B), dim3(64), 0, state, (long long)L, valid_dev, o.tiles, F);
    FD_LAUNCH(La, "loudness_pass2", k_loud_pass<true>, grid, dim3(256), 0, wav, (long long)L, valid_dev, o.tiles, state, part, peakbits,
              (double)rate, F);
    FD_LAUNCH(La, "loudness_gate", k_loud_gate, dim3(B), dim3(256), 0, (long long)L, valid_dev, o.tiles, (const double *)part,
              (const unsigned int *)peakbits, z, o.zpitch, o.zoff, (double)rate, normalize ? 1 : 0, target, rec);
    const unsigned gx = (unsigned)((L + 256 * 8 - 1) / (256 * 8));
    if (out_f32)
        FD_LAUNCH(La, "loudness_apply", k_loud_apply<float>, dim3(gx, B), dim3(256), 0, wav, (long long)L, valid_dev, (const fd_loudness *)rec, out_f32);
    if (out_pcm)
        FD_LAUNCH(La, "loudness_apply", k_loud_apply<int16_t>, dim3(gx, B), dim3(256), 0, wav, (long long)L, valid_dev, (const fd_loudness *)rec,
                  out_pcm);
    return hipSuccess;
}

}  // namespace fdk
