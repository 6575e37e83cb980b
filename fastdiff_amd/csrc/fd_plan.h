// fd_plan.h -- the two decisions of a denoiser step that more than one module has to know, each in one place: the layout of the
// range-flag words (host and device) and which kernel variant every stage launches under a StepMode and a weight set.  Part of
// fd_internal.h, which includes it behind the definitions it reads (fd::NBLK / LAYERS, DevWeights, StepMode); plain host code, no HIP call.
#pragma once

namespace fd {
// Words of Workspace::range_flag.  Word i: "an operand of the fp16x2 launch of stage i did not fit fp16 in this step" (zeroed every
// step); PREV + i: the same of the previous sampler step (skip_after_previous_overflow); STICKY + i: OR over all steps since the last
// clear (what option fallback = host reads back).  fd_read_tap("range_flags") hands the first WORDS out by number.
namespace flags {
constexpr int GEMM = 0;                                                                        // predictor GEMM (raised by the producer of its image)
__host__ __device__ constexpr int lvc(int block, int layer) { return 1 + block * LAYERS + layer; }      // 1 .. 12
__host__ __device__ constexpr int dblock(int d) { return 1 + NBLK * LAYERS + d; }              // 13 .. 15
__host__ __device__ constexpr int convt(int n) { return dblock(NBLK) + n; }                    // 16 .. 18: ConvTranspose of block n
constexpr int KP_FRONT = convt(NBLK);                                                          // 19: predictor front
constexpr int WORDS = 32;
constexpr int PREV = WORDS, STICKY = 2 * WORDS;
// The stages the host found flagged -> the stages a redo runs on fp32: the predictor front feeds the GEMM, so both go.
inline unsigned with_dependents(unsigned flagged) { return ((flagged >> KP_FRONT) & 1u) ? (flagged | (1u << GEMM)) : flagged; }
}  // namespace flags
}  // namespace fd

// How a stage that has an fp16x2 kernel and an fp32 one is launched (StepMode: inline_fallback, fp32_mask)
enum Pipe { PIPE_F16_THEN_F32, PIPE_F16_ONLY, PIPE_F32_ONLY };
enum GemmForm { GEMM_FP32, GEMM_DIRECT, GEMM_WINO16, GEMM_WINO32 };

// Everything a step's drivers decide from (mode, weights), resolved once per fd_forward / per piece of steps (behind fd_settle_refresh:
// the *_ok bits are stale while a refresh is pending).  What one launch leaves for another is a field here, so producer and consumer
// read the same bit.
struct StepPlan {
    Pipe pipe[fd::flags::KP_FRONT + 1];      // by flag word
    GemmForm gemm;                   // the fp16x2 GEMM's form, or GEMM_FP32 when pipe[GEMM] is fp32-only
    bool front_writes_h_image;       // the fp16-pipe predictor front writes the direct GEMM's piece image of h itself (no k_h_split)
    bool fuse_up[fd::NBLK];          // the block's ConvTranspose runs inside its first LVC layer (k_lvc_h2<.., UP>): blocks 1 and 2, both
                                     // stages fp16x2-only; x never goes to HBM and back in between
    bool fuse_final;                 // the last LVC layer (block 2, layer 3) leaves the final_conv sums in eps_acc; fast_final then adds
                                     // the bias and updates x.  Off when someone wants to look at the block output (taps)
};

inline StepPlan plan_step(const StepMode &m, const DevWeights &w)
{
    using namespace fd::flags;
    StepPlan p;
    auto set = [&](int word, bool f16_possible) {
        p.pipe[word] = !f16_possible || ((m.fp32_mask >> word) & 1u) ? PIPE_F32_ONLY : (m.inline_fallback ? PIPE_F16_THEN_F32 : PIPE_F16_ONLY);
    };
    set(GEMM, m.gemm_f16 && w.gemm_f16_ok);
    set(KP_FRONT, m.conv_f16 && w.kpf_f16_ok);
    for (int n = 0; n < fd::NBLK; ++n) {
        set(dblock(n), m.conv_f16 && w.dblock_f16_ok);
        set(convt(n), m.conv_f16 && w.convt_f16_ok);
        for (int l = 0; l < fd::LAYERS; ++l) set(lvc(n, l), m.lvc_f16 && w.lvc_f16_ok && (n > 0 || m.lvc_h8_mfma));      // hop 8: option lvc_h8
    }
    const bool wino = m.gemm_wino && w.gemm_w_ok;
    p.gemm = p.pipe[GEMM] == PIPE_F32_ONLY ? GEMM_FP32 : (!wino ? GEMM_DIRECT : (m.gemm_tile16 ? GEMM_WINO16 : GEMM_WINO32));
    // the Winograd form builds its own image (k_h_wino) and the fp32 GEMM reads the front's fp32 h
    p.front_writes_h_image = m.fast[ST_KP_FRONT] && p.pipe[KP_FRONT] != PIPE_F32_ONLY && p.gemm == GEMM_DIRECT;
    for (int n = 0; n < fd::NBLK; ++n)
        p.fuse_up[n] = m.fuse_up && n >= 1 && m.fast[ST_CONVT] && m.fast[ST_LVC] && p.pipe[convt(n)] == PIPE_F16_ONLY &&
                       p.pipe[lvc(n, 0)] == PIPE_F16_ONLY;
    p.fuse_final = m.fast[ST_LVC] && m.fast[ST_FINAL] && !m.keep_taps && m.fuse_final && p.pipe[lvc(fd::NBLK - 1, fd::LAYERS - 1)] != PIPE_F32_ONLY;
    return p;
}

// One stage's "fp16x2 kernel, then its fp32 twin" as its driver launches it:
//   if (s.f16) FD_LAUNCH(L, name, <fp16x2 kernel>, ..., s.flag, ...);
//   if (s.f32) FD_LAUNCH(L, s.label(name, "<stage>_fp32_fallback"), <fp32 kernel>, ..., s.run_if, ...);
struct Twin {
    bool f16, f32;
    int *flag;              // the stage's word: raised by the fp16x2 kernel
    const int *run_if;      // for the fp32 kernel: behind a twin it exits at once unless the flag is up; alone (null) it is the stage
    const char *label(const char *own, const char *fallback) const { return f16 ? fallback : own; }      // the fp32 launch's profile row
};
// f16_on: false when the stage's fp16x2-side launch is off for a reason of its own (fast_final: nothing fused into the last LVC layer)
inline Twin twin_of(const StepPlan &p, int word, int *range_flag, bool f16_on = true)
{
    const bool f16 = f16_on && p.pipe[word] != PIPE_F32_ONLY;
    return {f16, !f16 || p.pipe[word] != PIPE_F16_ONLY, range_flag + word, f16 ? range_flag + word : nullptr};
}
