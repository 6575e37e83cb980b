// step_plan_check.cpp -- plan_step (fd_plan.h) walked on the host over its whole input space, asserting what the stage drivers rely on:
//   * a word set in fp32_mask gives PIPE_F32_ONLY, and PIPE_F16_ONLY occurs only without the inline fallback;
//   * a twin launches at least one of its two kernels, hands out the stage's own word, and gives the fp32 kernel a run_if exactly
//     when the fp16x2 kernel runs in front of it;
//   * fuse_up[n] implies n >= 1 and that both convt(n) and lvc(n, 0) are fp16x2-only (the fused kernel has no fp32 twin);
//   * front_writes_h_image implies the direct form and that neither the front nor the GEMM is fp32-only (producer and consumer exist);
//   * a Winograd form implies gemm_w_ok, GEMM_FP32 goes with an fp32-only GEMM word and with nothing else;
//   * fuse_final implies lvc(2, 3) is not fp32-only, no taps, and both the LVC and the final stage on the fast set;
//   * the flag names reproduce the numbering 0, 1..12, 13..15, 16..18, 19 that fd_read_tap("range_flags") hands out.
// The space: fast[] all fast / each single stage naive / all naive; every combination of the nine option bits; both values of
// inline_fallback; fp32_mask 0, each single word 0..19, all; every combination of the six *_ok bits.
// No GPU, no HIP call.  Build and run under the host sanitizers:
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -Iinclude -Ifastdiff_amd/csrc tools/step_plan_check.cpp -o step_plan_check && ./step_plan_check
#include <cstdio>

#include "fd_internal.h"

using namespace fd::flags;

static long long failures = 0;
#define CHECK(cond)                                                                                        \
    do {                                                                                                   \
        if (!(cond)) {                                                                                     \
            if (failures < 20) std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);                  \
            ++failures;                                                                                    \
        }                                                                                                  \
    } while (0)

static void check_numbering()
{
    static_assert(GEMM == 0 && KP_FRONT == 19 && WORDS == 32 && PREV == 32 && STICKY == 64, "flag words");
    int next = 1;
    for (int n = 0; n < fd::NBLK; ++n)
        for (int l = 0; l < fd::LAYERS; ++l) CHECK(lvc(n, l) == next++);
    CHECK(next == 13);
    for (int d = 0; d < fd::NBLK; ++d) CHECK(dblock(d) == next++);
    for (int n = 0; n < fd::NBLK; ++n) CHECK(convt(n) == next++);
    CHECK(next == KP_FRONT);
    CHECK(with_dependents(1u << KP_FRONT) == ((1u << KP_FRONT) | (1u << GEMM)));
    CHECK(with_dependents(1u << lvc(2, 3)) == (1u << lvc(2, 3)) && with_dependents(0) == 0);
    std::printf("numbering: ok\n");
}

static void check_plan(const StepMode &m, const DevWeights &w)
{
    const StepPlan p = plan_step(m, w);
    static int words[WORDS];
    for (int i = 0; i <= KP_FRONT; ++i) {
        if ((m.fp32_mask >> i) & 1u) CHECK(p.pipe[i] == PIPE_F32_ONLY);
        if (p.pipe[i] == PIPE_F16_ONLY) CHECK(!m.inline_fallback);
        const Twin s = twin_of(p, i, words);
        CHECK((s.f16 || s.f32) && s.flag == words + i && s.run_if == (s.f16 ? words + i : nullptr));
        CHECK(s.f16 == (p.pipe[i] != PIPE_F32_ONLY) && s.f32 == (p.pipe[i] != PIPE_F16_ONLY));
    }
    for (int n = 0; n < fd::NBLK; ++n)
        if (p.fuse_up[n]) CHECK(n >= 1 && p.pipe[convt(n)] == PIPE_F16_ONLY && p.pipe[lvc(n, 0)] == PIPE_F16_ONLY);
    if (p.front_writes_h_image) CHECK(p.gemm == GEMM_DIRECT && p.pipe[KP_FRONT] != PIPE_F32_ONLY && p.pipe[GEMM] != PIPE_F32_ONLY);
    if (p.gemm == GEMM_WINO16 || p.gemm == GEMM_WINO32) CHECK(w.gemm_w_ok);
    CHECK((p.gemm == GEMM_FP32) == (p.pipe[GEMM] == PIPE_F32_ONLY));
    const int last = lvc(fd::NBLK - 1, fd::LAYERS - 1);
    if (p.fuse_final) CHECK(p.pipe[last] != PIPE_F32_ONLY && !m.keep_taps && m.fast[ST_LVC] && m.fast[ST_FINAL]);
    // fast_final's twin: the update behind a fused last layer, k_final as the stage itself or as its fallback
    const Twin f = twin_of(p, last, words, p.fuse_final);
    CHECK(f.f16 == p.fuse_final && (f.f16 || f.f32) && f.f32 == (!p.fuse_final || m.inline_fallback));
}

int main()
{
    check_numbering();
    long long n = 0;
    DevWeights w;
    for (int fs = 0; fs < ST_COUNT + 2; ++fs)                    // all fast, stage fs - 1 naive, all naive
        for (unsigned opt = 0; opt < (1u << 9); ++opt)
            for (int inl = 0; inl < 2; ++inl)
                for (int mk = 0; mk < 22; ++mk)                      // 0, each single word, all
                    for (unsigned ok = 0; ok < (1u << 6); ++ok) {
                        StepMode m;
                        for (int i = 0; i < ST_COUNT; ++i) m.fast[i] = fs == 0 || (fs <= ST_COUNT && i != fs - 1);
                        m.gemm_f16 = opt & 1; m.gemm_wino = opt & 2; m.gemm_tile16 = opt & 4; m.lvc_f16 = opt & 8; m.conv_f16 = opt & 16;
                        m.lvc_h8_mfma = opt & 32; m.fuse_final = opt & 64; m.fuse_up = opt & 128; m.keep_taps = opt & 256;
                        m.inline_fallback = inl != 0;
                        m.fp32_mask = mk == 0 ? 0u : (mk == 21 ? (1u << (KP_FRONT + 1)) - 1 : 1u << (mk - 1));
                        w.dblock_f16_ok = ok & 1; w.lvc_f16_ok = ok & 2; w.kpf_f16_ok = ok & 4; w.gemm_f16_ok = ok & 8; w.gemm_w_ok = ok & 16;
                        w.convt_f16_ok = ok & 32;
                        check_plan(m, w);
                        ++n;
                    }
    std::printf("plan: %lld combinations: %s\n", n, failures ? "FAIL" : "ok");
    return failures ? 1 : 0;
}
