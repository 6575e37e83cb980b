// fd_kernels_mcd.hip -- mel-cepstral distortion with time alignment on the device (include/fastdiff_hip_ext.h: fd_cepstra, fd_dtw,
// fd_mcd_measure, which define the computation; csrc/fd_mcd.h: the constants and index ranges).
//
//   k_cepstra<TACO>   grid (T_pitch, B), one workgroup = one frame: mel_frame (fd_kernels_melframe.h, the code k_mel_frontend runs) leaves
//                     the 80 log-mel values in threads 0 .. 79; they go to LDS as natural logarithms, and thread d < n_coef forms c_{d+1}
//                     as one fmaf chain over ascending j from its row of the DCT table, which the workgroup has copied to LDS.  A frame
//                     behind the row's own T writes zeros, a tacotron row of at most 512 samples NaN, a frame with a sample under its window
//                     that is not finite NaN.  No mel reaches memory.
//   k_dtw<DP>         ONE WORKGROUP PER PAIR, 256 threads = FD_DTW_ROWS rows of a at a time.  Thread r keeps row i0 + r of a in DP
//                     registers (zeros behind D: a zero difference adds nothing) and is at column j = s - r in step s.  b lies in LDS
//                     [d][slot], slot = j mod (ROWS + COLS), loaded COLS columns at a time in the phase of the step before they are
//                     first needed (the slots they take held columns no thread needs any more: fd_mcd.h tile_at).  The cell above,
//                     (i - 1, j), is thread r - 1's value of the step before: a cross-lane move inside a wavefront, a double-buffered
//                     LDS slot from the last lane of the wavefront before, and for thread 0 the bottom row of the block before, which
//                     went through the scratch and is staged with b.  The diagonal cell is the cell above of the step before, the
//                     left one the thread's own last value.  One barrier per step.  Each cell carries (D in float64, cells, diagonal
//                     steps) from the predecessor it chose, so the thread that finishes (Ta - 1, Tb - 1) writes the record.  With
//                     align_out the directions are kept, two bits per cell, and thread 0 walks them back at the end.
//   k_mcd_finish      one workgroup per pair: mcd_linear in a fixed order, the statuses, the 48-byte record.
//
// Workgroups never wait for each other.  No order depends on B or on where the pair lies in the batch, and there are no atomics on
// values: a record is bit-identical alone, in a ragged batch, at any ld and from call to call.
#include "fd_internal.h"
#include "fd_kernels.h"
#include "fd_kernels_common.h"
#include "fd_kernels_melframe.h"

namespace fdk {

constexpr int DT_ROWS = fdm::ROWS, DT_COLS = fdm::COLS, DT_RING = fdm::RING, DT_WAVES = fdm::WAVES;
static_assert(DT_ROWS == FD_DTW_ROWS && DT_COLS == FD_DTW_COLS && fdm::MAX_COEF == FD_MCD_MAX_COEF, "the exported constants are the kernels'");
static_assert(fdm::MAX_FRAMES == FD_MCD_MAX_FRAMES && fdm::MAX_ALIGN_CELLS == FD_DTW_MAX_ALIGN_CELLS, "the exported limits are the host's");
static_assert(sizeof(fd_dtw_rec) == 32 && sizeof(fd_mcd) == 48 && sizeof(fd_mcd_config) == 8, "the sizes the header states");
static_assert(DT_ROWS == 256 && fdm::WAVE == 64, "256-thread workgroups of 64-lane wavefronts");

__device__ __forceinline__ float quiet_nanf() { return __int_as_float(0x7FC00000); }
__device__ __forceinline__ bool bits_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

template <bool TACO>
__global__ void __launch_bounds__(256) k_cepstra(const float *__restrict__ wav, long long L, const long long *__restrict__ lens, float *__restrict__ cep,
                                                 long long T_pitch, int n_coef, const float *__restrict__ tab, const int *__restrict__ fb_lo,
                                                 const int *__restrict__ fb_n, const int *__restrict__ fb_off, const float *__restrict__ fb_w,
                                                 const float *__restrict__ dct)
{
    __shared__ MelFrameLds s;
    __shared__ float dl[fdm::MAX_COEF * fdm::MELS], ml[fdm::MELS];
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const long long n = own_len(lens, b, L);
    const long long T = 1 + n / fdm::HOP;
    float *out = cep + ((long long)b * T_pitch + t) * n_coef;
    if (t >= T || (TACO && n <= fdm::TACO_SHORT)) {        // (the whole workgroup)
        if (tid < n_coef) out[tid] = t >= T ? 0.0f : quiet_nanf();
        return;
    }
    for (int e = tid; e < n_coef * fdm::MELS; e += 256) dl[e] = dct[e];
    const float v = mel_frame<TACO>(s, wav + (long long)b * L, n, t, tab, fb_lo, fb_n, fb_off, fb_w, tid);
    bool nf = false;                                       // a sample under the window that is not finite (the front-end's floor would take it for silence)
#pragma unroll
    for (int j = 0; j < 4; ++j) nf |= !bits_finite(s.xw[j * 256 + tid]);
    const int any_nf = __syncthreads_or(nf);
    if (tid < fdm::MELS) ml[tid] = TACO ? v : __fmul_rn(v, 2.302585093f);
    __syncthreads();
    if (tid < n_coef) {
        const float *row = dl + tid * fdm::MELS;
        float acc = 0.0f;
#pragma unroll 8
        for (int j = 0; j < fdm::MELS; ++j) acc = fmaf(row[j], ml[j], acc);
        out[tid] = any_nf ? quiet_nanf() : acc;
    }
}

struct DtwArgs {
    const float *a, *b;
    int D;
    long long ld, pitch_a, pitch_b;
    const long long *fa, *fb;
    fd_dtw_rec *rec;
    int *align;
    long long align_pitch;
    double *botD;              // [B][2][bot_pitch]: the bottom row of a block for the next one ...
    int2 *botLN;               // ... with its cells and diagonal steps
    long long bot_pitch;
    unsigned char *codes;      // null, or [B][code_stride] bytes
    long long code_stride;
};

template <int DP>
__global__ void __launch_bounds__(256) k_dtw(DtwArgs A)
{
    __shared__ float bs[DP * DT_RING];
    __shared__ double upD[DT_RING];
    __shared__ int upL[DT_RING], upN[DT_RING];
    __shared__ double edD[2][DT_WAVES];
    __shared__ int edL[2][DT_WAVES], edN[2][DT_WAVES];
    __shared__ int bad;
    static_assert(sizeof(float) * DP * DT_RING + (sizeof(double) + 2 * sizeof(int)) * (DT_RING + 2 * DT_WAVES) + sizeof(int) == fdm::dtw_lds_bytes(DP), "fd_mcd.h states this workgroup's LDS");
    const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int D = A.D;
    const long long ld = A.ld;
    const long long Ta = own_len(A.fa, pair, A.pitch_a), Tb = own_len(A.fb, pair, A.pitch_b);
    const float *__restrict__ ap = A.a + (long long)pair * A.pitch_a * ld;
    const float *__restrict__ bp = A.b + (long long)pair * A.pitch_b * ld;
    int *al = A.align ? A.align + (long long)pair * A.align_pitch : nullptr;

    // the pre-scan: a feature that is not finite
    if (tid == 0) bad = 0;
    __syncthreads();
    {
        bool nf = false;
        for (long long i = tid; i < Ta; i += 256)
            for (int d = 0; d < D; ++d) nf |= !bits_finite(ap[i * ld + d]);
        for (long long j = tid; j < Tb; j += 256)
            for (int d = 0; d < D; ++d) nf |= !bits_finite(bp[j * ld + d]);
        if (nf) atomicOr(&bad, 1);
    }
    __syncthreads();
    if (bad) {                                             // (the whole workgroup)
        if (al)
            for (long long i = tid; i < A.align_pitch; i += 256) al[i] = -1;
        if (tid == 0) {
            fd_dtw_rec r;
            r.cost = quiet_nan();
            r.path_len = r.n_diag = 0;
            r.frames_a = (int)Ta; r.frames_b = (int)Tb;
            r.status = FD_MCD_NONFINITE; r.reserved = 0;
            A.rec[pair] = r;
        }
        return;
    }

    double *botD = A.botD + (long long)pair * 2 * A.bot_pitch;
    int2 *botLN = A.botLN + (long long)pair * 2 * A.bot_pitch;
    unsigned char *codes = A.codes ? A.codes + (long long)pair * A.code_stride : nullptr;
    const long long cpitch = (Tb + 3) / 4;
    const long long nblk = (Ta + DT_ROWS - 1) / DT_ROWS;

    // columns [lo, hi) of b, and of the bottom row of block k - 1, into their ring slots
    auto load_tile = [&](long long lo, long long hi, long long k) {
        const int cols = (int)(hi - lo);
        for (int e = tid; e < cols * DP; e += 256) {
            const int c = e / DP, d = e - c * DP;
            const long long j = lo + c;
            bs[d * DT_RING + (int)(j % DT_RING)] = d < D ? bp[j * ld + d] : 0.0f;
        }
        if (k > 0 && tid < cols) {
            const long long j = lo + tid;
            const int sl = (int)(j % DT_RING);
            const long long at = ((k - 1) & 1) * A.bot_pitch + j;
            const int2 ln = botLN[at];
            upD[sl] = botD[at]; upL[sl] = ln.x; upN[sl] = ln.y;
        }
    };

    for (long long k = 0; k < nblk; ++k) {
        const long long i0 = k * DT_ROWS, left = Ta - i0;
        const int nr = (int)(left < DT_ROWS ? left : DT_ROWS);
        const long long i = i0 + tid;
        const bool row_on = tid < nr;
        const bool to_next = k + 1 < nblk && tid == nr - 1;          // this row is the next block's row above
        float ar[DP];
#pragma unroll
        for (int d = 0; d < DP; ++d) ar[d] = (row_on && d < D) ? ap[i * ld + d] : 0.0f;
        load_tile(0, Tb < DT_COLS ? Tb : DT_COLS, k);      // (the last step of the block before ended with a barrier)
        __syncthreads();
        double curD = 0.0, dgD = 0.0;                      // this thread's last cell (the left one); the cell above of the step before
        int curL = 0, curN = 0, dgL = 0, dgN = 0;
        unsigned pk = 0;
        int sl = tid == 0 ? 0 : DT_RING - tid;              // the slot of column s - r while it is >= 0
        const long long S = Tb + nr - 1;
        for (long long s = 0; s < S; ++s) {
            const long long j = s - tid;
            // the cell above: (i - 1, j), thread r - 1's value of the step before
            double uD = __shfl_up(curD, 1);
            int uL = __shfl_up(curL, 1), uN = __shfl_up(curN, 1);
            if (lane == 0) {
                if (wave > 0) { const int q = (int)((s + 1) & 1); uD = edD[q][wave - 1]; uL = edL[q][wave - 1]; uN = edN[q][wave - 1]; }
                else if (k > 0 && j < Tb) { uD = upD[sl]; uL = upL[sl]; uN = upN[sl]; }
            }
            if (row_on && j >= 0 && j < Tb) {
                float acc = 0.0f;
#pragma unroll
                for (int d = 0; d < DP; ++d) { const float df = ar[d] - bs[d * DT_RING + sl]; acc = fmaf(df, df, acc); }
                const double c = (double)sqrtf(acc);
                const bool hu = i > 0, hl = j > 0, hd = hu && hl;
                double bD = 0.0;
                int bL = 0, bN = 0;
                unsigned dir = 0;
                if (hd) { bD = dgD; bL = dgL; bN = dgN + 1; }
                if (hu && (!hd || uD < bD)) { bD = uD; bL = uL; bN = uN; dir = 1; }
                if (hl && (!hu || curD < bD)) { bD = curD; bL = curL; bN = curN; dir = 2; }
                curD = c + bD; curL = bL + 1; curN = bN;
                if (codes) {
                    pk |= dir << (2 * (int)(j & 3));
                    if ((j & 3) == 3 || j == Tb - 1) { codes[i * cpitch + (j >> 2)] = (unsigned char)pk; pk = 0; }
                }
                if (to_next) { const long long at = (k & 1) * A.bot_pitch + j; botD[at] = curD; botLN[at] = make_int2(curL, curN); }
                if (i == Ta - 1 && j == Tb - 1) {
                    fd_dtw_rec r;
                    r.cost = curD; r.path_len = curL; r.n_diag = curN;
                    r.frames_a = (int)Ta; r.frames_b = (int)Tb;
                    r.status = FD_MCD_OK; r.reserved = 0;
                    A.rec[pair] = r;
                }
            }
            dgD = uD; dgL = uL; dgN = uN;
            if (lane == 63) { const int q = (int)(s & 1); edD[q][wave] = curD; edL[q][wave] = curL; edN[q][wave] = curN; }
            if (++sl == DT_RING) sl = 0;
            if ((s + 1) % DT_COLS == 0 && s + 1 < Tb) load_tile(s + 1, s + 1 + DT_COLS < Tb ? s + 1 + DT_COLS : Tb, k);
            __syncthreads();
        }
    }
    if (!al) return;
    __threadfence();
    __syncthreads();
    for (long long i = Ta + tid; i < A.align_pitch; i += 256) al[i] = -1;
    if (tid != 0) return;
    long long i = Ta - 1, j = Tb - 1;
    for (;;) {                                             // at most Ta + Tb - 1 cells: i + j falls with every step
        al[i] = (int)j;
        if (i == 0 && j == 0) break;
        unsigned c = (codes[i * cpitch + (j >> 2)] >> (2 * (int)(j & 3))) & 3u;
        if (i == 0) c = 2;
        else if (j == 0) c = 1;
        if (c == 0) { --i; --j; } else if (c == 1) --i; else --j;
    }
}

__global__ void __launch_bounds__(256) k_mcd_finish(const float *__restrict__ ca, const float *__restrict__ cb, int D, long long pitch_a, long long pitch_b,
                                                    const long long *__restrict__ fa, const long long *__restrict__ fb, const long long *__restrict__ na,
                                                    long long La, const long long *__restrict__ nb, long long Lb, int taco,
                                                    const fd_dtw_rec *__restrict__ dtw, fd_mcd *__restrict__ rec)
{
    __shared__ double red[256];
    const int pair = blockIdx.x, tid = threadIdx.x;
    const long long Ta = own_len(fa, pair, pitch_a), Tb = own_len(fb, pair, pitch_b), T = Ta < Tb ? Ta : Tb;
    const float *__restrict__ a = ca + (long long)pair * pitch_a * D, *__restrict__ b = cb + (long long)pair * pitch_b * D;
    const fd_dtw_rec w = dtw[pair];
    const bool is_short = taco && (own_len(na, pair, La) <= fdm::TACO_SHORT || own_len(nb, pair, Lb) <= fdm::TACO_SHORT);
    const bool ok = !is_short && w.status == FD_MCD_OK;
    double sum = 0.0;
    if (ok)
        for (long long i = tid; i < T; i += 256) {
            float acc = 0.0f;
            for (int d = 0; d < D; ++d) { const float df = a[i * D + d] - b[i * D + d]; acc = fmaf(df, df, acc); }
            sum += (double)sqrtf(acc);
        }
    red[tid] = sum;
    __syncthreads();
    if (tid != 0) return;
    sum = 0.0;
    for (int t = 0; t < 256; ++t) sum += red[t];
    fd_mcd r;
    r.mcd_dtw = r.mcd_linear = r.cost = quiet_nan();
    r.path_len = r.n_diag = 0;
    r.frames_clean = (int)Ta; r.frames_degraded = (int)Tb;
    r.status = is_short ? FD_MCD_SHORT : w.status;
    r.reserved = 0;
    if (ok) {
        r.cost = w.cost; r.path_len = w.path_len; r.n_diag = w.n_diag;
        r.mcd_dtw = fdm::K_DB * w.cost / (double)w.path_len;
        r.mcd_linear = fdm::K_DB * sum / (double)T;
    }
    rec[pair] = r;
}

// The scratch buffer: four count slots of MAX_B, then the bottom rows, the alignment records, the direction codes and the two cepstra
struct McdLayout { size_t counts[4], botD, botLN, rec, codes, cep[2], total; };
static McdLayout mcd_layout(int B, long long bot_pitch, long long code_stride, long long cep_floats_a, long long cep_floats_b)
{
    McdLayout o{};
    Carve cv;
    for (int q = 0; q < 4; ++q) o.counts[q] = cv.take(sizeof(long long) * fdm::MAX_B);
    o.botD = cv.take(sizeof(double) * 2 * (size_t)B * (size_t)bot_pitch);
    o.botLN = cv.take(sizeof(int2) * 2 * (size_t)B * (size_t)bot_pitch);
    o.rec = cv.take(sizeof(fd_dtw_rec) * (size_t)B);
    o.codes = cv.take((size_t)B * (size_t)code_stride);
    o.cep[0] = cv.take(sizeof(float) * (size_t)cep_floats_a);
    o.cep[1] = cv.take(sizeof(float) * (size_t)cep_floats_b);
    o.total = cv.at;
    return o;
}

size_t mcd_scratch_bytes(int B, long long bot_pitch, long long code_stride, long long cep_floats_a, long long cep_floats_b)
{
    return mcd_layout(B, bot_pitch, code_stride, cep_floats_a, cep_floats_b).total;
}

long long *mcd_count_slot(void *scratch, int which) { return reinterpret_cast<long long *>(static_cast<char *>(scratch) + mcd_layout(1, 0, 0, 0, 0).counts[which]); }

float *mcd_cep_slot(void *scratch, int B, long long bot_pitch, long long code_stride, long long cep_floats_a, long long cep_floats_b, int which)
{
    return reinterpret_cast<float *>(static_cast<char *>(scratch) + mcd_layout(B, bot_pitch, code_stride, cep_floats_a, cep_floats_b).cep[which]);
}

fd_dtw_rec *mcd_rec_slot(void *scratch, int B, long long bot_pitch, long long code_stride)
{
    return reinterpret_cast<fd_dtw_rec *>(static_cast<char *>(scratch) + mcd_layout(B, bot_pitch, code_stride, 0, 0).rec);
}

hipError_t cepstra(const Launch &La, const float *wav, int B, long long L, const long long *lens_dev, int n_coef, const float *dct, float *cep,
                   long long T_pitch)
{
    const MelTables &m = La.ctx->mel[La.ctx->mel_variant];
    const dim3 grid((unsigned)T_pitch, (unsigned)B);
    if (La.ctx->mel_variant == MEL_TACOTRON)
        FD_LAUNCH(La, "cepstra_tacotron", k_cepstra<true>, grid, dim3(256), 0, wav, L, lens_dev, cep, T_pitch, n_coef, m.tab, m.fb_lo, m.fb_n, m.fb_off, m.fb_w, dct);
    else
        FD_LAUNCH(La, "cepstra", k_cepstra<false>, grid, dim3(256), 0, wav, L, lens_dev, cep, T_pitch, n_coef, m.tab, m.fb_lo, m.fb_n, m.fb_off, m.fb_w, dct);
    return hipSuccess;
}

hipError_t dtw(const Launch &La, const float *a, const float *b, int B, int D, long long ld, long long pitch_a, long long pitch_b,
               const long long *fa_dev, const long long *fb_dev, fd_dtw_rec *rec, int *align, long long align_pitch, long long code_stride, void *scratch)
{
    const McdLayout o = mcd_layout(B, pitch_b, code_stride, 0, 0);
    char *base = static_cast<char *>(scratch);
    DtwArgs A{};
    A.a = a; A.b = b; A.D = D; A.ld = ld; A.pitch_a = pitch_a; A.pitch_b = pitch_b; A.fa = fa_dev; A.fb = fb_dev;
    A.rec = rec; A.align = align; A.align_pitch = align_pitch;
    A.botD = reinterpret_cast<double *>(base + o.botD);
    A.botLN = reinterpret_cast<int2 *>(base + o.botLN);
    A.bot_pitch = pitch_b;
    A.codes = align ? reinterpret_cast<unsigned char *>(base + o.codes) : nullptr;
    A.code_stride = code_stride;
    if (fdm::padded_d(D) == 16)
        FD_LAUNCH(La, "dtw_16", k_dtw<16>, dim3(B), dim3(256), 0, A);
    else
        FD_LAUNCH(La, "dtw_40", k_dtw<fdm::MAX_COEF>, dim3(B), dim3(256), 0, A);
    return hipSuccess;
}

hipError_t mcd_finish(const Launch &La, const float *ca, const float *cb, int B, int D, long long pitch_a, long long pitch_b, const long long *fa_dev,
                      const long long *fb_dev, const long long *na_dev, long long Lc, const long long *nb_dev, long long Ld, const fd_dtw_rec *dtw_rec,
                      fd_mcd *rec)
{
    FD_LAUNCH(La, "mcd_finish", k_mcd_finish, dim3(B), dim3(256), 0, ca, cb, D, pitch_a, pitch_b, fa_dev, fb_dev, na_dev, Lc, nb_dev, Ld,
              La.ctx->mel_variant == MEL_TACOTRON ? 1 : 0, dtw_rec, rec);
    return hipSuccess;
}

}  // namespace fdk
