// fd_api.cpp -- host side of libfastdiff_hip.so, the inference boundary (include/fastdiff_hip.h): context, workspace, the denoiser step
// sequence, the hipGraph-replayed reverse loop, options.  The state_dict ingestion (weight-norm fold + repack): fd_weights.cpp; the rows
// next to the path and the hooks: fd_api_ext.cpp (fastdiff_hip_ext.h); the training operators: fd_api_train.cpp (fastdiff_hip_train.h).
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "fd_kernels.h"
#include "fd_host.h"

std::string g_create_error;

// 256-byte rows of the predictor GEMM's fp16 image per utterance: the direct form's (gx_rows: whole item windows + 2 halo rows) or the
// Winograd form's (gw_pairs pair rows of four such rows each), whichever is larger -- both from the kernels' own definitions (fd_kernels.h)
static inline int gx_rows_host(int T) { return std::max(fdk_fast::gx_rows(T), fdk_fast::gw_pairs(T) * (fdk_fast::GW_ROWB / fdk_fast::GX_ROWB)); }

// ------------------------------------------------------------------------------------------------
// profiling helpers (declared in fd_internal.h)
// ------------------------------------------------------------------------------------------------
bool fd_prof_stamps(const fdk::Launch &L, const char *name, hipEvent_t *e0, hipEvent_t *e1)
{
    fd_context *c = L.ctx;
    if (c->profile != 1 || L.capturing) return false;
    hipEvent_t ev[2];
    for (int i = 0; i < 2; ++i) {
        if (!c->event_pool.empty()) { ev[i] = c->event_pool.back(); c->event_pool.pop_back(); }
        else if (hipEventCreate(&ev[i]) != hipSuccess) return false;
    }
    ProfEntry pe;
    pe.name = name;
    pe.e0 = *e0 = ev[0]; pe.e1 = *e1 = ev[1];
    c->prof_pending.push_back(pe);
    return true;
}

void fd_prof_begin(const fdk::Launch &L, const char *name)
{
    fd_context *c = L.ctx;
    if (c->profile != 2 || L.capturing) return;
    ProfEntry pe;
    pe.name = name;
    hipEvent_t ev[2];
    for (int i = 0; i < 2; ++i) {
        if (!c->event_pool.empty()) { ev[i] = c->event_pool.back(); c->event_pool.pop_back(); }
        else if (hipEventCreate(&ev[i]) != hipSuccess) return;
    }
    pe.e0 = ev[0]; pe.e1 = ev[1];
    hipEventRecord(pe.e0, L.stream);
    c->prof_pending.push_back(pe);
}

void fd_prof_end(const fdk::Launch &L)
{
    fd_context *c = L.ctx;
    if (c->profile != 2 || L.capturing || c->prof_pending.empty()) return;
    hipEventRecord(c->prof_pending.back().e1, L.stream);
}

void fd_prof_drain(fd_context *c)
{
    for (auto &pe : c->prof_pending) {
        float ms = 0.0f;
        if (hipEventSynchronize(pe.e1) == hipSuccess && hipEventElapsedTime(&ms, pe.e0, pe.e1) == hipSuccess) {
            auto &acc = c->prof_acc[pe.name];
            acc.first += 1;
            acc.second += ms;
        }
        c->event_pool.push_back(pe.e0);
        c->event_pool.push_back(pe.e1);
    }
    c->prof_pending.clear();
}

// ------------------------------------------------------------------------------------------------
// C ABI: lifecycle
// ------------------------------------------------------------------------------------------------
extern "C" {

const char *fd_version(void) { return "fastdiff_hip 0.2 (gfx950)"; }
// 2: fd_sample settles its own range check before returning unless option defer_check = 1 (revision 1: always deferred)
int fd_abi_revision(void) { return 2; }

int fd_default_config(fd_config *cfg)
{
    if (!cfg) return FD_ERR_INVALID;
    memset(cfg, 0, sizeof(*cfg));
    cfg->audio_channels = 1; cfg->inner_channels = 32; cfg->cond_channels = 80; cfg->n_upsample = 3;
    cfg->upsample_ratios[0] = 8; cfg->upsample_ratios[1] = 8; cfg->upsample_ratios[2] = 4;
    cfg->lvc_layers_each_block = 4; cfg->lvc_kernel_size = 3; cfg->kpnet_hidden_channels = 64; cfg->kpnet_conv_size = 3;
    cfg->diffusion_step_embed_dim_in = 128; cfg->diffusion_step_embed_dim_mid = 512; cfg->diffusion_step_embed_dim_out = 512;
    cfg->use_weight_norm = 1;
    return FD_OK;
}

const char *fd_last_error(fd_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

static void release_handle(fd_context *h);

int fd_create(const fd_config *cfg, int device, fd_handle *out)
{
    fd_context *nullh = nullptr;
    if (!cfg || !out) FD_FAIL(nullh, FD_ERR_INVALID, "fd_create: null argument");
    fd_config ref;
    fd_default_config(&ref);
    // base.yaml's architecture (every shipped YAML) runs on the tuned gfx950 kernel set; any other configuration the reference
    // constructor accepts (FastDiff_model.py:13-26) on the runtime-shaped kernels of fd_generic.hip
    bool is_base = cfg->audio_channels == ref.audio_channels && cfg->inner_channels == ref.inner_channels &&
                   cfg->cond_channels == ref.cond_channels && cfg->n_upsample == ref.n_upsample &&
                   cfg->lvc_layers_each_block == ref.lvc_layers_each_block && cfg->lvc_kernel_size == ref.lvc_kernel_size &&
                   cfg->kpnet_hidden_channels == ref.kpnet_hidden_channels && cfg->kpnet_conv_size == ref.kpnet_conv_size &&
                   cfg->diffusion_step_embed_dim_in == ref.diffusion_step_embed_dim_in &&
                   cfg->diffusion_step_embed_dim_mid == ref.diffusion_step_embed_dim_mid &&
                   cfg->diffusion_step_embed_dim_out == ref.diffusion_step_embed_dim_out;
    for (int i = 0; is_base && i < ref.n_upsample; ++i) is_base = cfg->upsample_ratios[i] == ref.upsample_ratios[i];
    if (!is_base) {
        std::string why;
        if (fdg::validate(*cfg, why) != FD_OK) FD_FAIL(nullh, FD_ERR_UNSUPPORTED, "fd_create: %s", why.c_str());
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        FD_FAIL(nullh, FD_ERR_HIP, "fd_create: no HIP device available (%s); there is no CPU fallback", hipGetErrorString(e));
    if (device < 0 || device >= ndev) FD_FAIL(nullh, FD_ERR_INVALID, "fd_create: device %d out of range (0..%d)", device, ndev - 1);
    FD_HIP(nullh, hipSetDevice(device));
    fd_context *c = new fd_context();
    c->cfg = *cfg;
    c->device = device;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) c->num_cus = prop.multiProcessorCount;
    }
    // every resource of the handle lives in *c from the moment it exists, so one failure path (fd_destroy's own release code) frees
    // whatever was created before the failing call
    auto fail = [&](hipError_t err) {
        g_create_error = std::string("fd_create: ") + hipGetErrorString(err);
        release_handle(c);
        return FD_ERR_HIP;
    };
    if ((e = hipStreamCreateWithFlags(&c->cap_stream, hipStreamNonBlocking)) != hipSuccess) return fail(e);
    if ((e = hipMalloc(&c->scratch, 65536)) != hipSuccess) return fail(e);
    if ((e = hipHostMalloc(reinterpret_cast<void **>(&c->flags_host), 256, hipHostMallocDefault)) != hipSuccess) return fail(e);
    memset(c->flags_host, 0, 256);
    if ((e = hipEventCreateWithFlags(&c->flags_done, hipEventDisableTiming)) != hipSuccess) return fail(e);
    if ((e = hipEventCreateWithFlags(&c->flags_done2, hipEventDisableTiming)) != hipSuccess) return fail(e);
    // the staging ring is allocated here (64 KB per slot covers the step table and a few thousand utterances): a call only
    // allocates pinned memory again for a larger batch than that
    for (auto &sl : c->stage) {
        if ((e = hipHostMalloc(reinterpret_cast<void **>(&sl.host), 65536, hipHostMallocDefault)) != hipSuccess) return fail(e);
        sl.cap = 65536;
    }
    if (!is_base) fdg::create(c);
    *out = c;
    return FD_OK;
}

static void free_workspace(fd_context *c)
{
    Workspace &w = c->ws;
    void *ptrs[] = {w.noise, w.embed_h2, w.a[0], w.a[1], w.a[2], w.a[3], w.kp_h0, w.kp_hA, w.kp_hB, w.kpack, w.h_f16, w.range_flag, w.lens_dev, w.uid_dev, w.off_dev, w.xsave, w.xA, w.xB,
                    w.xtap[0], w.xtap[1], w.xtap[2], w.mel, w.mel_rep, w.x, w.eps_acc, w.steps, w.params};
    for (void *p : ptrs)
        if (p) hipFree(p);
    w = Workspace();
}

// Destroys the retired graphs whose last launch has completed (all of them when `wait`: the caller has synchronised the device).
static void reap_retired(fd_context *c, bool wait)
{
    for (size_t i = 0; i < c->retired.size();) {
        fd_context::RetiredGraph &r = c->retired[i];
        if (!wait && r.done && hipEventQuery(r.done) != hipSuccess) { (void)hipGetLastError(); ++i; continue; }
        if (r.exec) hipGraphExecDestroy(r.exec);
        if (r.graph) hipGraphDestroy(r.graph);
        if (r.done) hipEventDestroy(r.done);
        c->retired.erase(c->retired.begin() + i);
    }
}

// Drops every captured graph.  The caller has just synchronised the device (workspace growth, fd_commit_weights, fd_destroy): no
// replay is queued any more.  (An option does not drop graphs: the mode it changes is part of every graph's key.)
void drop_graph(fd_context *c)
{
    for (auto &g : c->graphs) {
        if (g.exec) hipGraphExecDestroy(g.exec);
        if (g.graph) hipGraphDestroy(g.graph);
    }
    c->graphs.clear();
    reap_retired(c, true);
}

// Frees everything a handle owns (each member is null until created): the tail of fd_destroy and the failure path of fd_create.
static void release_handle(fd_context *h)
{
    fdg::destroy(h);
    if (h->flags_host) hipHostFree(h->flags_host);
    if (h->flags_done) hipEventDestroy(h->flags_done);
    if (h->flags_done2) hipEventDestroy(h->flags_done2);
    for (auto ev : h->event_pool) hipEventDestroy(ev);
    drop_graph(h);
    free_workspace(h);
    if (h->weight_arena) hipFree(h->weight_arena);
    if (h->refresh_dev) hipFree(h->refresh_dev);
    if (h->refresh_bad) hipHostFree(h->refresh_bad);
    if (h->refresh_done) hipEventDestroy(h->refresh_done);
    if (h->scratch) hipFree(h->scratch);
    for (Scratch *s : {&h->lvc_scratch, &h->kconv_scratch, &h->cconv_scratch, &h->span_scratch, &h->ring_scratch, &h->step_scratch, &h->loud_scratch, &h->stoi_scratch, &h->pitch_scratch, &h->spectral_scratch, &h->gl_scratch, &h->nnls_scratch, &h->bins_scratch, &h->mcd_scratch, &h->trim_scratch, &h->pwg_scratch})
        if (s->p) hipFree(s->p);
    for (auto &sl : h->stage) {
        if (sl.host) hipHostFree(sl.host);
        if (sl.done) hipEventDestroy(sl.done);
    }
    for (void *p : h->tables) hipFree(p);
    if (h->ev_switch) hipEventDestroy(h->ev_switch);
    if (h->cap_stream) hipStreamDestroy(h->cap_stream);
    delete h;
}

int fd_destroy(fd_handle h)
{
    if (!h) return FD_ERR_INVALID;
    hipSetDevice(h->device);
    fd_settle(h);
    hipDeviceSynchronize();
    fd_prof_drain(h);
    release_handle(h);
    return FD_OK;
}

// ------------------------------------------------------------------------------------------------
// workspace
// ------------------------------------------------------------------------------------------------
// Buffers scale with three quantities of a call: B (per-utterance arrays), B*T (every activation, the predicted kernels) and
// B*gx_rows(T) (the GEMM's fp16 image, padded per utterance).  Capacity is tracked in exactly those terms, so a handle that served
// (B=64, T=864) and then meets (B=1, T=20000) needs room for max(64*864, 20000) frames -- not for 64 x 20000.
static hipError_t allocate_workspace(fd_context *h, int64_t capB, int64_t frames, int64_t rows, int64_t pframes, int64_t prows, int64_t plens,
                                     size_t *total_out)
{
    h->embed_valid = false;          // a fresh noise table
    Workspace &w = h->ws;
    const size_t f = sizeof(float), FL = (size_t)frames * fd::HOPT;      // FL: samples of all utterances together
    size_t total = 0;
    auto alloc = [&](float **p, size_t n) -> hipError_t {
        total += n * f;
        hipError_t e1 = hipMalloc(reinterpret_cast<void **>(p), n * f);
        // zero once: with ragged batches (lens) tiles behind an utterance are never written, and nothing a later kernel
        // stages next to them (range checks run over whole tiles) should meet NaN bit patterns of a fresh allocation
        return e1 == hipSuccess ? hipMemset(*p, 0, n * f) : e1;
    };
    hipError_t e = hipSuccess;
#define WS(p, n) if (e == hipSuccess) e = alloc(&(p), (n))
    WS(w.noise, (size_t)1024 * capB * fd::NBLK * fd::COND);
    WS(w.embed_h2, (size_t)std::max<int64_t>(1024, capB) * fd::E_OUT);
    WS(w.a[0], fd::C * FL); WS(w.a[1], fd::C * FL / 4); WS(w.a[2], fd::C * FL / 32); WS(w.a[3], (size_t)fd::C * frames);
    // the predictor's buffers: their own capacities (a hoisted predictor holds N reverse steps: fd_internal.h)
    WS(w.kp_h0, (size_t)fd::NBLK * fd::HID * pframes); WS(w.kp_hA, (size_t)fd::NBLK * fd::HID * pframes);
    WS(w.kp_hB, (size_t)fd::NBLK * fd::HID * pframes);
    WS(w.kpack, (size_t)fd::NBLK * pframes * fd::KREC);
    WS(w.h_f16, (size_t)fd::NBLK * prows * (fdk_fast::GX_ROWB / f) + 1024);      // + slack for the rounded-up last DMA
    WS(w.mel_rep, (size_t)fd::COND * pframes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&w.lens_dev), sizeof(int) * (size_t)std::max<int64_t>(plens, 64));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&w.uid_dev), sizeof(unsigned long long) * (size_t)std::max<int64_t>(capB, 64));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&w.range_flag), 512);
    if (e == hipSuccess) e = hipMemset(w.range_flag, 0, 512);
    WS(w.xA, fd::C * FL); WS(w.xB, fd::C * FL);
    WS(w.xtap[0], fd::C * FL / 32); WS(w.xtap[1], fd::C * FL / 4); WS(w.xtap[2], fd::C * FL);
    WS(w.mel, (size_t)fd::COND * frames); WS(w.x, FL); WS(w.xsave, FL); WS(w.eps_acc, FL); WS(w.steps, (size_t)std::max<int64_t>(capB, 64));
#undef WS
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&w.params), sizeof(StepParams));
    if (e == hipSuccess) e = hipMemset(w.params, 0, sizeof(StepParams));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&w.off_dev), sizeof(long long) * (size_t)std::max<int64_t>(capB, 64));
    *total_out = total;
    return e;
}

static bool workspace_fits(const fd_context *h, int B, int T, int pmult)
{
    const Workspace &w = h->ws;
    const int64_t frames = (int64_t)B * T, rows = (int64_t)B * gx_rows_host(T);
    return w.B >= B && w.frames >= frames && w.rows >= rows && w.params && w.pframes >= frames * pmult && w.prows >= rows * pmult &&
           w.plens >= (int64_t)B * pmult;
}

static int ensure_workspace(fd_context *h, int B, int T, int pmult = 1)
{
    Workspace &w = h->ws;
    const int64_t frames = (int64_t)B * T, rows = (int64_t)B * gx_rows_host(T);
    if (workspace_fits(h, B, T, pmult)) return FD_OK;
    FD_HIP(h, hipDeviceSynchronize());
    drop_graph(h);
    // grow to the largest of each quantity seen so far, so that alternating shapes settle; if that does not fit, this call's own
    // needs alone are tried before giving up
    const int64_t own[6] = {B, frames, rows, frames * pmult, rows * pmult, (int64_t)B * pmult};
    const int64_t seen[6] = {w.B, w.frames, w.rows, w.pframes, w.prows, w.plens};
    int64_t want[2][6];
    bool same = true;
    for (int i = 0; i < 6; ++i) {
        want[0][i] = std::max(own[i], seen[i]);
        // a stream of requests of growing length (the reference CLI's pattern) would otherwise re-allocate -- a device synchronisation,
        // every buffer freed and allocated again, every graph dropped -- once per new maximum: grow by at least a quarter
        if (own[i] > seen[i] && seen[i] > 0) want[0][i] = std::max(own[i], seen[i] + seen[i] / 4);
        want[1][i] = own[i];
        same = same && want[0][i] == want[1][i];
    }
    size_t total = 0;
    hipError_t e = hipSuccess;
    for (int attempt = 0; attempt < 2; ++attempt) {
        free_workspace(h);
        e = allocate_workspace(h, want[attempt][0], want[attempt][1], want[attempt][2], want[attempt][3], want[attempt][4], want[attempt][5], &total);
        if (e == hipSuccess) {
            w.B = (int)want[attempt][0]; w.frames = want[attempt][1]; w.rows = want[attempt][2];
            w.pframes = want[attempt][3]; w.prows = want[attempt][4]; w.plens = want[attempt][5]; w.bytes = total;
            return FD_OK;
        }
        (void)hipGetLastError();
        if (same) break;
    }
    free_workspace(h);
    FD_FAIL(h, FD_ERR_HIP, "workspace allocation for B=%d T=%d (%.1f MB) failed: %s", B, T, total / 1e6, hipGetErrorString(e));
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// stage dispatch + the denoiser step
// ------------------------------------------------------------------------------------------------
namespace fdk {

// fast | naive (option kernels.<stage>): each stage's one dispatch
static hipError_t first_conv(const Launch &L, const StepIO &io, int B, int T)
{
    return L.mode->fast[ST_FIRST] ? fast_first_conv(L, io, B, T) : naive_first_conv(L, io, B, T);
}
static hipError_t dblock(const Launch &L, const StepIO &io, int d, int B, int T)
{
    return L.mode->fast[ST_DBLOCK] ? fast_dblock(L, d, B, T, io.x_in) : naive_dblock(L, d, B, T);
}
static hipError_t convt(const Launch &L, int n, const float *x_in, float *x_out, int B, int Lin)
{
    return L.mode->fast[ST_CONVT] ? fast_convt(L, n, x_in, x_out, B, Lin) : naive_convt(L, n, x_in, x_out, B, Lin);
}
// cur -> cur: the fast layer writes `other` and the two change places; the naive one works in place with `other` as scratch
static hipError_t lvc_layer(const Launch &L, const StepIO &io, int n, int i, float *&cur, float *&other, const float *skip, int B, int T)
{
    if (!L.mode->fast[ST_LVC]) return naive_lvc_layer(L, n, i, cur, skip, other, B, T);
    const hipError_t e = fast_lvc_layer(L, io, n, i, cur, skip, other, B, T);
    std::swap(cur, other);
    return e;
}
// The predictor (front + GEMM) over `entries` batch entries: a step's own B utterances, or a hoisted batch of (step, utterance) entries
static hipError_t predictor(const Launch &L, const StepIO &io, int entries, int T)
{
    const hipError_t e = L.mode->fast[ST_KP_FRONT] ? fast_kp_front(L, io, entries, T) : naive_kp_front(L, io, entries, T);
    if (e != hipSuccess) return e;
    return L.mode->fast[ST_KP_GEMM] ? fast_kp_gemm(L, entries, T) : naive_kp_gemm(L, entries, T);
}

// One TimeAware_LVCBlock (modules.py:190-218) given the packed kernels of kp_gemm.  x_in: [B,32,Lin].
static hipError_t lvc_block_run(const Launch &L, const StepIO &io, int n, const float *x_in, int B, int T, float **x_out)
{
    Workspace &ws = L.ctx->ws;
    const int Lin = T * (fd::hop(n) / fd::ratio(n));
    float *cur = (x_in == ws.xA) ? ws.xB : ws.xA;
    float *other = (cur == ws.xA) ? ws.xB : ws.xA;
    const float *skip = ws.a[2 - n];
    // fuse_up: the up-sampler runs inside the first layer, which reads x_in and writes the other buffer
    const bool fuse_up = L.plan->fuse_up[n];
    hipError_t e = fuse_up ? fast_lvc_layer(L, io, n, 0, x_in, skip, cur, B, T, true) : convt(L, n, x_in, cur, B, Lin);
    for (int i = fuse_up ? 1 : 0; i < fd::LAYERS && e == hipSuccess; ++i) e = lvc_layer(L, io, n, i, cur, other, skip, B, T);
    if (e == hipSuccess && L.mode->keep_taps)
        e = hipMemcpyAsync(ws.xtap[n], cur, sizeof(float) * (size_t)B * fd::C * T * fd::hop(n), hipMemcpyDeviceToDevice, L.stream);
    *x_out = cur;
    return e;
}

static hipError_t run_step(const Launch &L, const StepIO &io, int B, int T)
{
    Workspace &ws = L.ctx->ws;
    hipError_t e;
    // the reference's order of statements: down path (first conv, DBlocks), predictor (front + GEMM), the three LVC blocks.  With a
    // hoisted predictor (hoist_np > 1) front + GEMM of all N steps ran in front of the loop (sample_core).  Other orders and a second
    // stream were measured and did not pay (LABBOOK.md: overlap = gemm | paths, order = split | predictor).
    const bool hoisted = L.mode->hoist_np > 1;
    // (round 6, measured and not kept: first_conv -- whose output a0 has no reader before the last block -- on a side branch of the
    // graph next to the DBlocks, joined in front of block 2, bit-identical: B=8 +0.5 %, B=1 +6 %; LABBOOK R6.7)
    if ((e = first_conv(L, io, B, T)) != hipSuccess) return e;
    for (int d = 0; d < fd::NBLK; ++d)
        if ((e = dblock(L, io, d, B, T)) != hipSuccess) return e;
    if (!hoisted && (e = predictor(L, io, B, T)) != hipSuccess) return e;
    float *x = ws.a[3];
    for (int n = 0; n < fd::NBLK; ++n) {
        float *xo = nullptr;
        if ((e = lvc_block_run(L, io, n, x, B, T, &xo)) != hipSuccess) return e;
        x = xo;
    }
    if (L.mode->fast[ST_FINAL]) return fast_final(L, io, x, B, T);
    // naive tail: eps into the free ping-pong buffer (or the caller's), then the separate update kernel
    float *eps = io.sampler ? ((x == ws.xA) ? ws.xB : ws.xA) : io.eps_out;
    if ((e = naive_final_eps(L, x, eps, B, T)) != hipSuccess) return e;
    if (io.sampler) return naive_update(L, ws.x, eps, (int64_t)B * T * fd::HOPT);
    return hipSuccess;
}

}  // namespace fdk

// ------------------------------------------------------------------------------------------------
// C ABI: compute
// ------------------------------------------------------------------------------------------------
extern "C" {


static int check_common(fd_handle h, int B, int T, const char *who)
{
    if (!h) return FD_ERR_INVALID;
    if (!h->committed) FD_FAIL(h, FD_ERR_STATE, "%s: weights not committed (call fd_commit_weights after fd_set_weight)", who);
    if (B <= 0 || T <= 0) FD_FAIL(h, FD_ERR_INVALID, "%s: B=%d T=%d must be positive", who, B, T);
    if ((int64_t)B * T * fdg::hop_total(h) * (h->gen ? h->cfg.inner_channels : fd::C) >= (int64_t)1 << 31)
        FD_FAIL(h, FD_ERR_INVALID, "%s: B*T too large for one call (B=%d, T=%d); split the batch", who, B, T);
    FD_HIP(h, hipSetDevice(h->device));
    return fd_settle_refresh(h);
}

// Pinned staging (fd_context::stage): the next slot of the ring with room for `bytes`, free to be written by the host.
int fd_stage_acquire(fd_handle h, size_t bytes, fd_context::StageSlot **out)
{
    fd_context::StageSlot &sl = h->stage[h->stage_next++ % fd_context::STAGE_SLOTS];
    if (sl.done) FD_HIP(h, hipEventSynchronize(sl.done));             // the uploads that last used this slot (8 calls ago)
    else FD_HIP(h, hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    if (sl.cap < bytes) {
        if (sl.host) hipHostFree(sl.host);
        sl.host = nullptr; sl.cap = 0;
        const size_t cap = (bytes + 4095) & ~(size_t)4095;
        FD_HIP(h, hipHostMalloc(reinterpret_cast<void **>(&sl.host), cap, hipHostMallocDefault));
        sl.cap = cap;
    }
    *out = &sl;
    return FD_OK;
}
// ... and the mark behind the copies that read it
int fd_stage_commit(fd_handle h, fd_context::StageSlot *sl, hipStream_t stream)
{
    FD_HIP(h, hipEventRecord(sl->done, stream));
    return FD_OK;
}
// host bytes -> the device array `dev` through one slot (the call does not wait for the copy)
int fd_stage_upload(fd_handle h, const void *src, size_t bytes, void *dev, hipStream_t stream)
{
    fd_context::StageSlot *sl = nullptr;
    const int rc = fd_stage_acquire(h, bytes, &sl);
    if (rc != FD_OK) return rc;
    memcpy(sl->host, src, bytes);
    FD_HIP(h, hipMemcpyAsync(dev, sl->host, bytes, hipMemcpyHostToDevice, stream));
    return fd_stage_commit(h, sl, stream);
}

// One stream at a time per handle: a call on another stream than the previous one first settles what is pending there and then makes
// the new stream wait for the tail of the handle's last call (workspace, embedding rows and step parameters are reused from call to
// call).  The tail is an EVENT recorded at the end of every call (fd_mark_tail), not the old stream itself: the caller may have
// destroyed that stream since (its work done), and the runtime does not survive a call on a destroyed stream handle
// (tools/stream_switch_probe.py: a hipEventRecord there takes the process down); an event outlives its stream.
int fd_mark_tail(fd_handle h, hipStream_t s)
{
    if (!h->ev_switch) FD_HIP(h, hipEventCreateWithFlags(&h->ev_switch, hipEventDisableTiming));
    FD_HIP(h, hipEventRecord(h->ev_switch, s));
    h->tail_marked = true;
    return FD_OK;
}

int fd_follow_stream(fd_handle h, hipStream_t s)
{
    if (h->have_last_stream && h->last_stream != s) {
        const int rc = fd_settle(h);      // (a pending check may redo its call on the old stream: that stream must live until the call is settled)
        if (rc != FD_OK) return rc;
        if (h->tail_marked) FD_HIP(h, hipStreamWaitEvent(s, h->ev_switch, 0));
    }
    h->last_stream = s;
    h->have_last_stream = true;
    return FD_OK;
}

// `lens` (host, nullable): valid frames per utterance of a zero-padded batch, uploaded for the kernels from the pinned area `staged`;
// *ragged: they were (some utterance is shorter than T).
// reps: the hoisted predictor's batch holds every utterance once per reverse step (entry n * B + b): its lengths are staged that often
static int set_lens(fd_handle h, const int *lens, int B, int T, hipStream_t stream, const char *who, int *staged, bool *ragged_out, int reps = 1)
{
    *ragged_out = false;
    if (!lens) return FD_OK;
    bool ragged = false;
    for (int b = 0; b < B; ++b) {
        if (lens[b] < 1 || lens[b] > T) FD_FAIL(h, FD_ERR_INVALID, "%s: lens[%d] = %d outside [1, T=%d]", who, b, lens[b], T);
        ragged = ragged || lens[b] < T;
    }
    if (!ragged) return FD_OK;                       // every utterance fills the batch: same launches as without lens
    for (int i = ST_FIRST; i < ST_COUNT; ++i)      // (the step embedding has no time axis)
        if (!h->mode.fast[i])
            FD_FAIL(h, FD_ERR_UNSUPPORTED, "%s: a ragged batch (lens) needs the fast kernel set; the naive kernels (option kernels.<stage> = naive) "
                                           "compute the padded tensor and would silently ignore the lengths", who);
    for (int n = 0; n < reps; ++n) memcpy(staged + (size_t)n * B, lens, sizeof(int) * B);
    FD_HIP(h, hipMemcpyAsync(h->ws.lens_dev, staged, sizeof(int) * B * reps, hipMemcpyHostToDevice, stream));
    *ragged_out = true;
    return FD_OK;
}

int fd_forward(fd_handle h, const float *x, const float *mel, const float *steps, int B, int T, const int *lens,
               float *eps_out, void *stream)
{
    if (h) { h->noise_ids.clear(); h->noise_offs.clear(); }   // stream ids are for the next fd_sample only: a forward in between drops them
    int rc = check_common(h, B, T, "fd_forward");
    if (rc != FD_OK) return rc;
    if ((rc = fd_settle(h)) != FD_OK) return rc;
    if ((rc = fd_follow_stream(h, (hipStream_t)stream)) != FD_OK) return rc;
    h->embed_valid = false;                      // fd_forward writes its own rows into the same table
    if (!x || !mel || !steps || !eps_out) FD_FAIL(h, FD_ERR_INVALID, "fd_forward: null pointer");
    if (x == eps_out) FD_FAIL(h, FD_ERR_INVALID, "fd_forward: eps_out must not alias x");
    if (h->gen) {
        for (int b = 0; lens && b < B; ++b)
            if (lens[b] < 1 || lens[b] > T) FD_FAIL(h, FD_ERR_INVALID, "fd_forward: lens[%d] = %d outside [1, T=%d]", b, lens[b], T);
        if ((rc = fdg::forward(h, x, mel, steps, B, T, lens, eps_out, (hipStream_t)stream)) != FD_OK) return rc;
        h->last_B = B; h->last_T = T;
        return fd_mark_tail(h, (hipStream_t)stream);
    }
    if ((rc = ensure_workspace(h, B, T)) != FD_OK) return rc;
    StepMode mode = h->mode;      // a single forward: its fallbacks inline, its own predictor (the per-call fields' defaults)
    if (lens) {
        fd_context::StageSlot *sl = nullptr;
        if ((rc = fd_stage_acquire(h, sizeof(int) * B, &sl)) != FD_OK) return rc;
        if ((rc = set_lens(h, lens, B, T, (hipStream_t)stream, "fd_forward", reinterpret_cast<int *>(sl->host), &mode.ragged)) != FD_OK) return rc;
        if ((rc = fd_stage_commit(h, sl, (hipStream_t)stream)) != FD_OK) return rc;
    }
    const StepPlan plan = plan_step(mode, h->w);      // (behind check_common: the weights' *_ok bits are settled)
    fdk::Launch L = {h, (hipStream_t)stream, false, &mode, &plan};
    StepIO io = {x, mel, steps, eps_out, 0};
    hipError_t e = fdk::embed(L, io, B, 1);
    if (e == hipSuccess) e = fdk::clear_range_flags(L);
    if (e == hipSuccess) e = fdk::run_step(L, io, B, T);
    if (e != hipSuccess) FD_FAIL(h, FD_ERR_HIP, "fd_forward: kernel launch failed: %s", hipGetErrorString(e));
    h->last_B = B; h->last_T = T;
    return fd_mark_tail(h, (hipStream_t)stream);
}

static int resolve_pending(fd_handle h, unsigned *mask);
// Every entry point that touches device state first settles a pending fallback = host check (no-op otherwise).
int fd_settle(fd_handle h)
{
    if (!h->pending.active) return FD_OK;
    unsigned mask = 0;
    const int rc = resolve_pending(h, &mask);
    return rc < 0 ? rc : FD_OK;
}

// `count` consecutive denoiser steps of the current call on `stream`, starting at the device step counter: replayed from captured
// graphs of up to 8 steps (kept per (B, T, steps, mode): there are ~9 us between two graph launches, so a short schedule is one launch
// per call, a long one a series of 8-step launches and a shorter one for the remainder), or launched one by one (options graph = 0,
// profile = 1).  mode: the call's (fd_internal.h: StepMode).
static int enqueue_steps(fd_handle h, int B, int T, int count, const StepMode &mode, hipStream_t stream)
{
    Workspace &ws = h->ws;
    constexpr int CHUNK = 8;
    // hoist_chunk: a piece of `steps` steps has the predictor of its own steps in front of it, over steps * B (step, utterance) entries
    auto piece_mode = [&](int steps) {
        StepMode m = mode;
        if (m.hoist_chunk) m.hoist_np = steps;
        return m;
    };
    // between two steps of a piece the bookkeeping rides in the next step's first kernel -- when that kernel is the fast one.  (Not
    // across pieces: a piece predictor's front reads the embedding rows through the device step counter, which must stand at the
    // piece's first step.)
    const bool defer_advance = mode.fuse_advance && mode.fast[ST_FIRST];
    auto enqueue_piece = [&](const fdk::Launch &L, int steps) -> hipError_t {
        const int np = L.mode->hoist_chunk ? L.mode->hoist_np : 1;
        hipError_t e = hipSuccess;
        if (np > 1) e = fdk::predictor(L, {ws.x, ws.mel_rep, nullptr, nullptr, np}, B * np, T);
        for (int k = 0; k < steps && e == hipSuccess; ++k) {
            StepIO io = {ws.x, ws.mel, nullptr, nullptr, 1};
            io.hoist_step = L.mode->hoist_np > 1 ? k : 0;      // (hoisted: the piece is the whole call or one 8-step piece of it)
            io.advance = k > 0 && defer_advance;
            e = fdk::run_step(L, io, B, T);
            if (e == hipSuccess && !(k + 1 < steps && defer_advance)) e = fdk::advance_step(L);
        }
        return e;
    };
    if (!(h->use_graph && !h->profile)) {
        const int piece = mode.hoist_chunk ? CHUNK : count;
        for (int first = 0; first < count; first += piece) {
            const int steps = std::min(piece, count - first);
            const StepMode m = piece_mode(steps);
            const StepPlan plan = plan_step(m, h->w);
            const hipError_t e = enqueue_piece({h, stream, false, &m, &plan}, steps);
            if (e != hipSuccess) FD_FAIL(h, FD_ERR_HIP, "fd_sample: launch of steps %d.. failed: %s", first, hipGetErrorString(e));
        }
        return FD_OK;
    }
    // `reps` replays of the graph of a piece of `steps` steps, captured first if it is not cached.  Enqueued right away: a capture for
    // the next piece that evicts this graph records the retire event behind them.
    auto replay = [&](int steps, int reps) -> int {
        const StepMode m = piece_mode(steps);
        hipGraphExec_t ex = nullptr;
        for (auto &g : h->graphs)
            if (g.B == B && g.T == T && g.steps == steps && g.mode == m) {
                g.last_use = ++h->graph_clock;
                ex = g.exec;
                ++h->n_graph_hits;
                break;
            }
        if (!ex) {
            reap_retired(h, false);
            while (h->graphs.size() >= (size_t)std::max(1, h->max_graphs)) {
                // evict the least recently used one.  It may still be running (or be queued behind the work on `stream`): retired with
                // an event recorded here, destroyed by a later call once that event has completed -- no wait on this path
                size_t lru = 0;
                for (size_t i = 1; i < h->graphs.size(); ++i)
                    if (h->graphs[i].last_use < h->graphs[lru].last_use) lru = i;
                fd_context::RetiredGraph r = {h->graphs[lru].graph, h->graphs[lru].exec, nullptr};
                FD_HIP(h, hipEventCreateWithFlags(&r.done, hipEventDisableTiming));
                FD_HIP(h, hipEventRecord(r.done, stream));
                h->retired.push_back(r);
                h->graphs.erase(h->graphs.begin() + lru);
                ++h->n_graph_evictions;
            }
            ++h->n_graph_captures;
            FD_HIP(h, hipStreamBeginCapture(h->cap_stream, hipStreamCaptureModeThreadLocal));
            const StepPlan plan = plan_step(m, h->w);      // (the graph stays keyed on the mode: the plan follows from it and the weights)
            const hipError_t ec = enqueue_piece({h, h->cap_stream, true, &m, &plan}, steps);
            hipGraph_t g = nullptr;
            const hipError_t e2 = hipStreamEndCapture(h->cap_stream, &g);
            if (ec != hipSuccess || e2 != hipSuccess) {
                if (g) hipGraphDestroy(g);
                FD_FAIL(h, FD_ERR_HIP, "fd_sample: graph capture failed: %s", hipGetErrorString(ec != hipSuccess ? ec : e2));
            }
            const hipError_t e3 = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
            if (e3 != hipSuccess) {
                hipGraphDestroy(g);
                FD_FAIL(h, FD_ERR_HIP, "fd_sample: hipGraphInstantiate: %s", hipGetErrorString(e3));
            }
            h->graphs.push_back({B, T, steps, m, g, ex, ++h->graph_clock});
        }
        for (int r = 0; r < reps; ++r) FD_HIP(h, hipGraphLaunch(ex, stream));
        return FD_OK;
    };
    int rc = count >= CHUNK ? replay(CHUNK, count / CHUNK) : FD_OK;
    if (rc == FD_OK && count % CHUNK) rc = replay(count % CHUNK, 1);
    return rc;
}

static int sample_core(fd_handle h, const fd_context::SampleArgs &a, unsigned force_mask, long long ticket);

// Frames of the library's own buffers for a sample call of T frames (fd_context::t_bucket): T rounded up to the bucket when the call
// is replayed from graphs and every stage runs the kernel set that honours `lens`; T itself otherwise.
static int bucket_frames(const fd_context *h, int T)
{
    if (h->t_bucket <= 1 || !h->use_graph || h->profile || h->mode.keep_taps) return T;
    for (int i = ST_FIRST; i < ST_COUNT; ++i)
        if (!h->mode.fast[i]) return T;
    const int64_t tp = ((int64_t)T + h->t_bucket - 1) / h->t_bucket * h->t_bucket;
    return tp > 0x3fffffff ? T : (int)tp;
}

// How many reverse steps' kernels one predictor launch pair computes for this call: N (hoisted) or 1 (the predictor stays in the step)
static int hoist_mult(const fd_context *h, int B, int T, int N)
{
    if (h->hoist_mode == 0 || N < 2) return 1;
    if (!(h->mode.fast[ST_KP_FRONT] && h->mode.fast[ST_KP_GEMM] && h->mode.fast[ST_LVC]) || h->mode.keep_taps) return 1;
    const int np = std::min(N, 8);             // a longer schedule hoists per 8-step graph piece (StepMode::hoist_chunk)
    if (h->hoist_mode == 2) return np;
    return (int64_t)B * T <= 4096 ? np : 1;        // measured at T = 864: B = 1 -7.8 %, 2 -6.2 %, 3 -4.1 %, 4 -1.9 %, 8 and 16 +-0 (profiles/r03/s20_*)
}

// fallback = host: waits for the pending piece of work, looks at its range flags and, if one was raised, runs that piece again with
// the flagged stages on their fp32 kernels (and every other stage with its fallback inline: the second pass is always right) -- a
// lazily checked call (<= 8 steps) as a whole from its arguments, a piece of a long schedule from the saved x.
// Returns 1 if it redid the work, 0 if not; *mask receives the flagged stages (sticky for the rest of a long call).
static int resolve_call(fd_handle h, const fd_context::PendingCall &p, unsigned *mask)
{
    FD_HIP(h, hipEventSynchronize(p.slot ? h->flags_done2 : h->flags_done));
    const int *fl = h->flags_host + fd::flags::WORDS * p.slot;
    unsigned m = 0;
    for (int i = 0; i < fd::flags::WORDS; ++i)
        if (fl[i]) m |= 1u << i;
    m = fd::flags::with_dependents(m);
    *mask |= m;
    if (m == 0) return 0;
    h->redone_ring[h->redone_next++ % 16] = p.ticket;
    if (p.lazy) ++h->n_calls_redone;
    else { ++h->n_pieces_redone; h->call_fp32_mask |= *mask; }
    if (p.lazy) {
        const int rc = sample_core(h, p.args, *mask, p.ticket);
        return rc < 0 ? rc : 1;
    }
    Workspace &ws = h->ws;
    const size_t n_el = (size_t)p.B * p.T * fd::HOPT;
    FD_HIP(h, hipMemcpyAsync(ws.x, ws.xsave, sizeof(float) * n_el, hipMemcpyDeviceToDevice, p.stream));
    StepMode mode = p.mode;
    mode.fp32_mask = *mask;
    mode.inline_fallback = true;
    fdk::Launch L = {h, p.stream, false, &mode};
    hipError_t e = fdk::clear_range_flags(L, p.first);
    if (e != hipSuccess) FD_FAIL(h, FD_ERR_HIP, "fd_sample_check: %s", hipGetErrorString(e));
    int rc = enqueue_steps(h, p.B, p.T, p.count, mode, p.stream);
    if (rc != FD_OK) return rc;
    if (p.first + p.count == p.N) {
        e = fdk::copy_rows(L, p.out, (int64_t)p.T_io * fd::HOPT, ws.x, (int64_t)p.T * fd::HOPT, p.T_io * fd::HOPT, p.B);
        if (e != hipSuccess) FD_FAIL(h, FD_ERR_HIP, "fd_sample_check: %s", hipGetErrorString(e));
    }
    return 1;
}

static int resolve_pending(fd_handle h, unsigned *mask)
{
    fd_context::PendingCall p = h->pending;
    h->pending.active = false;
    return resolve_call(h, p, mask);
}

// One whole sample call on a.stream.  force_mask != 0: a redo (the flagged stages on fp32, every other fallback inline, nothing left
// pending); otherwise the handle's mode: in-graph fallbacks, or fallback = host (lazy for N <= 8, checked every 8 steps beyond).
static int sample_core(fd_handle h, const fd_context::SampleArgs &a, unsigned force_mask, long long ticket)
{
    int rc;
    // T: frames of the library's buffers (the caller's T_io rounded up to the bucket); the caller's tensors keep their dense T_io layout
    const int B = a.B, T_io = a.T, T = bucket_frames(h, a.T), N = a.N;
    const int64_t L_io = (int64_t)T_io * fd::HOPT, Lp = (int64_t)T * fd::HOPT;
    hipStream_t stream = a.stream;
    Workspace &ws = h->ws;
    const size_t n_el = (size_t)B * T * fd::HOPT;
    const std::vector<unsigned long long> &ids = a.ids;
    constexpr int CHUNK = 8;
    // this call's mode.  Hoisted predictor: one front + GEMM launch pair over the batch of np * B (step, utterance) entries -- in front
    // of the loop (N <= 8), or in front of each 8-step piece (hoist_chunk).  force_mask != 0 (a redo): every fallback inline
    StepMode mode = h->mode;
    const int np = hoist_mult(h, B, T, N);
    mode.hoist_np = np;
    mode.hoist_chunk = np > 1 && N > CHUNK;
    mode.fp32_mask = force_mask;
    mode.inline_fallback = force_mask != 0 || !h->host_fallback;
    std::vector<int> own_lens;                  // a bucketed call without `lens`: every utterance is T_io of the T frames long
    const int *lens_eff = a.has_lens ? a.lens.data() : nullptr;
    if (!lens_eff && T != T_io) { own_lens.assign(B, T_io); lens_eff = own_lens.data(); }
    // per-call parameters -> device block the captured kernels read.  Staged through the pinned ring: the call returns
    // without waiting for the stream, so the host prepares the next call while this one runs.
    {
        fd_context::StageSlot *sl = nullptr;
        const size_t off_lens = sizeof(StepParams), off_ids = off_lens + ((sizeof(int) * B * np + 7) & ~(size_t)7);
        const size_t off_offs = off_ids + sizeof(unsigned long long) * B;
        const bool has_offs = !ids.empty() && !a.offs.empty();
        if ((rc = fd_stage_acquire(h, off_offs + sizeof(long long) * B, &sl)) != FD_OK) return rc;
        if ((rc = set_lens(h, lens_eff, B, T, stream, "fd_sample", reinterpret_cast<int *>(sl->host + off_lens), &mode.ragged, np)) != FD_OK)
            return rc;
        if (!ids.empty()) {
            memcpy(sl->host + off_ids, ids.data(), sizeof(unsigned long long) * B);
            FD_HIP(h, hipMemcpyAsync(ws.uid_dev, sl->host + off_ids, sizeof(unsigned long long) * B, hipMemcpyHostToDevice, stream));
        }
        if (has_offs) {
            memcpy(sl->host + off_offs, a.offs.data(), sizeof(long long) * B);
            FD_HIP(h, hipMemcpyAsync(ws.off_dev, sl->host + off_offs, sizeof(long long) * B, hipMemcpyHostToDevice, stream));
        }
        StepParams *p = reinterpret_cast<StepParams *>(sl->host);
        memcpy(p->table, a.table.data(), sizeof(fd_step) * N);
        p->z = a.z; p->seq = a.seq_out; p->seed = a.seed; p->n_steps = N; p->ddim = a.ddim ? 1 : 0; p->step_idx = 0; p->l4 = T * (fd::HOPT / 4);
        p->uids = ids.empty() ? nullptr : ws.uid_dev;
        p->offs4 = has_offs ? ws.off_dev : nullptr;
        p->l4_io = T_io * (fd::HOPT / 4); p->n4_io = (long long)B * p->l4_io;
        // only the used prefix of the table plus the trailer needs to travel
        const size_t head = sizeof(fd_step) * N;
        FD_HIP(h, hipMemcpyAsync(ws.params, p, head, hipMemcpyHostToDevice, stream));
        const size_t off = offsetof(StepParams, z);
        FD_HIP(h, hipMemcpyAsync(reinterpret_cast<char *>(ws.params) + off, reinterpret_cast<const char *>(p) + off, sizeof(StepParams) - off,
                                 hipMemcpyHostToDevice, stream));
        if ((rc = fd_stage_commit(h, sl, stream)) != FD_OK) return rc;
    }
    fdk::Launch L = {h, stream, false, &mode};
    hipError_t e = fdk::copy_rows(L, ws.mel, T, a.mel, T_io, T_io, B * fd::COND);
    if (e == hipSuccess && a.x_T) e = fdk::copy_rows(L, ws.x, Lp, a.x_T, L_io, (int)L_io, B);
    if (e != hipSuccess) FD_FAIL(h, FD_ERR_HIP, "fd_sample: input copy failed: %s", hipGetErrorString(e));
    if (!a.x_T && (e = fdk::init_noise(L, ws.x, B, T * (fd::HOPT / 4), T_io * (fd::HOPT / 4), a.seed, ids.empty() ? nullptr : ws.uid_dev,
                                       ids.empty() || a.offs.empty() ? nullptr : ws.off_dev)) != hipSuccess)
        FD_FAIL(h, FD_ERR_HIP, "fd_sample: init_noise failed: %s", hipGetErrorString(e));
    if (a.seq_out && (e = fdk::copy_rows(L, a.seq_out, L_io, ws.x, Lp, (int)L_io, B)) != hipSuccess)
        FD_FAIL(h, FD_ERR_HIP, "fd_sample: sequence copy failed: %s", hipGetErrorString(e));
    // the waveform back into the caller's dense tensor
    auto copy_out = [&]() -> int {
        const hipError_t eo = fdk::copy_rows(L, a.out, L_io, ws.x, Lp, (int)L_io, B);
        if (eo != hipSuccess) FD_FAIL(h, FD_ERR_HIP, "fd_sample: output copy failed: %s", hipGetErrorString(eo));
        return FD_OK;
    };

    StepIO io = {ws.x, ws.mel, nullptr, nullptr, 1};
    {   // the embedding rows of this schedule: still in ws.noise from the previous call?
        std::vector<float> ts(N);
        for (int k = 0; k < N; ++k) ts[k] = a.table[k].t;
        if (!(h->embed_cache && h->embed_valid && h->embed_B == B && h->embed_t == ts)) {
            h->embed_valid = false;
            if ((e = fdk::embed(L, io, B, N)) != hipSuccess) FD_FAIL(h, FD_ERR_HIP, "fd_sample: embed failed: %s", hipGetErrorString(e));
            h->embed_t.swap(ts);
            h->embed_B = B;
            h->embed_valid = true;
        }
    }
    if ((e = fdk::clear_range_flags(L)) != hipSuccess) FD_FAIL(h, FD_ERR_HIP, "fd_sample: %s", hipGetErrorString(e));

    if (np > 1) {      // the mel once per predicted step: ONE launch (the lengths were staged that often by set_lens)
        const int64_t mel_n = (int64_t)B * fd::COND * T;
        if ((e = fdk::copy_rows(L, ws.mel_rep, T, ws.mel, T, T, B * fd::COND, np, mel_n)) != hipSuccess)
            FD_FAIL(h, FD_ERR_HIP, "fd_sample: mel replication failed: %s", hipGetErrorString(e));
    }
    if (np > 1 && !mode.hoist_chunk) {      // (hoist_chunk: enqueue_steps puts one in front of every piece)
        const StepPlan plan = plan_step(mode, h->w);      // (this piece is the whole call: the same plan as its steps')
        // "forward" addressing: batch entry n * B + b reads noise row n * B + b
        e = fdk::predictor({h, stream, false, &mode, &plan}, {ws.x, ws.mel_rep, nullptr, nullptr, 0}, B * N, T);
        if (e != hipSuccess) FD_FAIL(h, FD_ERR_HIP, "fd_sample: predictor launch failed: %s", hipGetErrorString(e));
    }
    if (force_mask != 0) {
        if ((rc = enqueue_steps(h, B, T, N, mode, stream)) != FD_OK) return rc;
        if ((rc = copy_out()) != FD_OK) return rc;
    } else if (h->host_fallback && N <= CHUNK) {
        // fallback = host, one graph launch: no fp32 launch trails the fp16x2 kernels; their flags accumulate on the device and travel
        // to the host behind the work.  Looked at lazily: by the next fd_sample after it has enqueued itself, or by fd_sample_check /
        // fd_sample_settle; a flagged call is then run again as a whole.
        if ((rc = enqueue_steps(h, B, T, N, mode, stream)) != FD_OK) return rc;
        const int slot = (int)(ticket & 1);
        FD_HIP(h, hipMemcpyAsync(h->flags_host + fd::flags::WORDS * slot, ws.range_flag + fd::flags::STICKY, sizeof(int) * fd::flags::WORDS, hipMemcpyDeviceToHost, stream));
        FD_HIP(h, hipEventRecord(slot ? h->flags_done2 : h->flags_done, stream));
        if ((rc = copy_out()) != FD_OK) return rc;      // provisional until checked
        h->pending.active = true; h->pending.lazy = true; h->pending.slot = slot; h->pending.ticket = ticket;
        h->pending.B = B; h->pending.T = T; h->pending.T_io = T_io; h->pending.N = N; h->pending.first = 0; h->pending.count = N; h->pending.out = a.out;
        h->pending.stream = stream; h->pending.args = a;
    } else if (h->host_fallback) {
        // a long schedule: each 8-step piece is checked (one stream synchronisation) before the next is enqueued, and redone from the
        // saved x with the flagged stages on their fp32 kernels once the host has seen them
        FD_HIP(h, hipMemcpyAsync(ws.xsave, ws.x, sizeof(float) * n_el, hipMemcpyDeviceToDevice, stream));
        unsigned mask = 0;
        for (int first = 0; first < N; first += CHUNK) {
            const int count = std::min(CHUNK, N - first);
            const bool last = first + count == N;
            ++h->n_pieces;
            if (mask != 0) ++h->n_pieces_fp32;
            if (first > 0 && mask == 0) FD_HIP(h, hipMemcpyAsync(ws.xsave, ws.x, sizeof(float) * n_el, hipMemcpyDeviceToDevice, stream));
            mode.fp32_mask = mask;
            mode.inline_fallback = mask != 0;
            if ((rc = enqueue_steps(h, B, T, count, mode, stream)) != FD_OK) return rc;
            if (mask != 0) continue;              // already on the safe path: nothing to look at
            FD_HIP(h, hipMemcpyAsync(h->flags_host, ws.range_flag + fd::flags::STICKY, sizeof(int) * fd::flags::WORDS, hipMemcpyDeviceToHost, stream));
            FD_HIP(h, hipEventRecord(h->flags_done, stream));
            h->pending.active = true; h->pending.lazy = false; h->pending.slot = 0; h->pending.ticket = ticket;
            h->pending.B = B; h->pending.T = T; h->pending.T_io = T_io; h->pending.N = N; h->pending.first = first; h->pending.count = count; h->pending.out = a.out;
            h->pending.stream = stream; h->pending.mode = mode;
            if (last) break;                      // the caller's fd_sample_check (or the next call on this handle) looks at it
            int redone = resolve_pending(h, &mask);
            if (redone < 0) return redone;
        }
        if ((rc = copy_out()) != FD_OK) return rc;      // (provisional while a check is pending)
    } else {
        if ((rc = enqueue_steps(h, B, T, N, mode, stream)) != FD_OK) return rc;
        if ((rc = copy_out()) != FD_OK) return rc;
    }
    h->last_B = B; h->last_T = T;
    return fd_mark_tail(h, stream);      // (also behind a redo: resolve_call comes through here)
}

int fd_sample(fd_handle h, const float *mel, int B, int T, const int *lens, const fd_step *table, int N, int ddim,
              const float *x_T, const float *z, uint64_t seed, float *out, float *seq_out, void *stream_)
{
    std::vector<unsigned long long> ids;
    std::vector<long long> offs;
    if (h) { ids.swap(h->noise_ids); offs.swap(h->noise_offs); }   // one-shot: fd_set_noise_streams applies to this call only, also when it fails below
    int rc = check_common(h, B, T, "fd_sample");
    if (rc != FD_OK) return rc;
    if ((rc = fd_follow_stream(h, (hipStream_t)stream_)) != FD_OK) return rc;
    if (h->gen) {      // a configuration other than base.yaml's: exact-fp32 kernels, nothing provisional, no graph
        if (!mel || !table || !out) FD_FAIL(h, FD_ERR_INVALID, "fd_sample: null pointer");
        if (N <= 0 || N > 1024) FD_FAIL(h, FD_ERR_INVALID, "fd_sample: N=%d outside 1..1024", N);
        if (!ids.empty() && (int)ids.size() != B) FD_FAIL(h, FD_ERR_INVALID, "fd_sample: fd_set_noise_streams gave %d stream ids but B=%d", (int)ids.size(), B);
        for (int b = 0; lens && b < B; ++b)
            if (lens[b] < 1 || lens[b] > T) FD_FAIL(h, FD_ERR_INVALID, "fd_sample: lens[%d] = %d outside [1, T=%d]", b, lens[b], T);
        if ((rc = fdg::sample(h, mel, B, T, lens, table, N, ddim, x_T, z, seed, ids, out, seq_out, (hipStream_t)stream_)) != FD_OK) return rc;
        ++h->ticket_counter;
        h->last_B = B; h->last_T = T;
        return fd_mark_tail(h, (hipStream_t)stream_);
    }
    // A lazily checked previous call (fallback = host, <= 8 steps) is looked at AFTER this call has enqueued its own work -- unless
    // this call cannot be lazy itself, or the workspace must grow first (that waits for the device anyway).
    const bool lazy = h->host_fallback && N >= 1 && N <= 8;
    const int Tp = bucket_frames(h, T);          // frames of the library's own buffers (t_bucket): what the workspace and the graphs are sized for
    if ((rc = check_common(h, B, Tp, "fd_sample")) != FD_OK) return rc;
    const int np = (N >= 1 && N <= 1024) ? hoist_mult(h, B, Tp, N) : 1;
    const bool ws_ok = workspace_fits(h, B, Tp, np);
    fd_context::PendingCall prev;
    if (lazy && ws_ok && h->pending.active && h->pending.lazy) {
        prev = h->pending;
        h->pending.active = false;
    } else if ((rc = fd_settle(h)) != FD_OK) return rc;
    auto finish_prev = [&]() -> int {
        if (!prev.active) return FD_OK;
        unsigned mask = 0;
        const fd_context::PendingCall cur = h->pending;      // a redo of the previous call must not disturb this call's record
        h->pending.active = false;
        const int r = resolve_call(h, prev, &mask);
        h->pending = cur;
        prev.active = false;
        return r < 0 ? r : FD_OK;
    };
    if (!mel || !table || !out) { finish_prev(); FD_FAIL(h, FD_ERR_INVALID, "fd_sample: null pointer"); }
    if (N <= 0 || N > 1024) { finish_prev(); FD_FAIL(h, FD_ERR_INVALID, "fd_sample: N=%d outside 1..1024", N); }
    if (!ids.empty() && (int)ids.size() != B) {
        finish_prev();
        FD_FAIL(h, FD_ERR_INVALID, "fd_sample: fd_set_noise_streams gave %d stream ids but B=%d", (int)ids.size(), B);
    }
    if (!offs.empty() && offs.size() != ids.size()) { finish_prev(); FD_FAIL(h, FD_ERR_INVALID, "fd_sample: noise offsets without their stream ids"); }
    for (int b = 0; lens && b < B; ++b)
        if (lens[b] < 1 || lens[b] > T) {
            finish_prev();
            FD_FAIL(h, FD_ERR_INVALID, "fd_sample: lens[%d] = %d outside [1, T=%d]", b, lens[b], T);
        }
    if ((rc = ensure_workspace(h, B, Tp, np)) != FD_OK) { finish_prev(); return rc; }
    fd_context::SampleArgs a;
    a.mel = mel; a.B = B; a.T = T; a.N = N; a.ddim = ddim;
    a.has_lens = lens != nullptr;
    if (lens) a.lens.assign(lens, lens + B);
    a.table.assign(table, table + N);
    a.x_T = x_T; a.z = z; a.seed = seed; a.out = out; a.seq_out = seq_out; a.stream = (hipStream_t)stream_;
    a.ids.swap(ids);
    a.offs.swap(offs);
    const long long ticket = ++h->ticket_counter;
    h->n_pieces = h->n_pieces_redone = h->n_pieces_fp32 = 0;
    h->call_fp32_mask = 0;
    rc = sample_core(h, a, 0u, ticket);
    const int rc_prev = finish_prev();
    h->last_B = B; h->last_T = Tp;               // (a redo of the previous call has just run with that call's shape)
    if (rc != FD_OK || rc_prev != FD_OK) return rc != FD_OK ? rc : rc_prev;
    // The contract of the reference call is "call, then read" (util.py:215-235): unless the caller opted into the pipelined check
    // (option defer_check = 1: tickets, fd_sample_check / fd_sample_settle), the range check of this call is settled before fd_sample
    // returns -- one wait for the call's own work and, if an operand left the fp16 range, the second pass on the fp32 kernels.
    if (!h->defer_check) return fd_settle(h);
    return FD_OK;
}

int64_t fd_sample_ticket(fd_handle h) { return h ? (int64_t)h->ticket_counter : FD_ERR_INVALID; }

// 1 if call `ticket` had to be redone on the fp32 kernels (now, or when a later fd_sample looked at it), 0 if not.
static int ticket_redone(fd_handle h, long long ticket)
{
    for (long long t : h->redone_ring)
        if (t == ticket && t != 0) return 1;
    return 0;
}

int fd_sample_settle(fd_handle h, int64_t ticket)
{
    if (!h) return FD_ERR_INVALID;
    if (ticket <= 0 || ticket > h->ticket_counter) FD_FAIL(h, FD_ERR_INVALID, "fd_sample_settle: unknown ticket %lld", (long long)ticket);
    if (h->pending.active && h->pending.ticket <= ticket) {
        FD_HIP(h, hipSetDevice(h->device));
        unsigned mask = 0;
        const int r = resolve_pending(h, &mask);
        if (r < 0) return r;
    }
    return ticket_redone(h, ticket);
}

int fd_sample_check(fd_handle h)
{
    if (!h) return FD_ERR_INVALID;
    if (!h->pending.active) return 0;
    FD_HIP(h, hipSetDevice(h->device));
    unsigned mask = 0;
    return resolve_pending(h, &mask);
}

int fd_set_noise_streams(fd_handle h, const uint64_t *stream_ids, int B)
{
    if (!h || B < 0 || (B > 0 && !stream_ids)) return FD_ERR_INVALID;
    h->noise_ids.assign(stream_ids, stream_ids + B);
    h->noise_offs.clear();
    return FD_OK;
}

// ------------------------------------------------------------------------------------------------
// options, taps, profile
// ------------------------------------------------------------------------------------------------
int fd_set_option(fd_handle h, const char *key, const char *value)
{
    if (!h || !key || !value) return FD_ERR_INVALID;
    {
        const int rcs = fd_settle(h);
        if (rcs != FD_OK) return rcs;
    }
    const std::string k(key), v(value);
    static const char *stage_names[ST_COUNT] = {"embed", "first", "dblock", "kp_front", "kp_gemm", "convt", "lvc", "final"};
    auto parse_mode = [&](bool &dst) -> int {
        if (v == "fast") dst = true;
        else if (v == "naive") dst = false;
        else FD_FAIL(h, FD_ERR_INVALID, "fd_set_option: %s expects fast|naive, got '%s'", key, value);
        return FD_OK;
    };
    if (k == "kernels") {
        bool m = true;
        int rc = parse_mode(m);
        if (rc != FD_OK) return rc;
        for (int i = 0; i < ST_COUNT; ++i) h->mode.fast[i] = m;
        return FD_OK;
    }
    if (k.compare(0, 8, "kernels.") == 0) {
        for (int i = 0; i < ST_COUNT; ++i)
            if (k.substr(8) == stage_names[i]) return parse_mode(h->mode.fast[i]);
        FD_FAIL(h, FD_ERR_INVALID, "fd_set_option: unknown stage '%s'", key);
    }
    // the options of two named values: set(h, value == a)
    static const struct { const char *key, *a, *b; void (*set)(fd_context *, bool); } choices[] = {
        {"gemm", "f16x2", "fp32", [](fd_context *c, bool a) { c->mode.gemm_f16 = a; }},
        {"gemm_form", "winograd", "direct", [](fd_context *c, bool a) { c->mode.gemm_wino = a; }},   // how the fp16x2 GEMM does its 3 taps
        {"gemm_tile", "16", "32", [](fd_context *c, bool a) { c->mode.gemm_tile16 = a; }},           // rows of the Winograd form's matrix tiles
        {"lvc", "f16x2", "fp32", [](fd_context *c, bool a) { c->mode.lvc_f16 = a; }},
        {"conv", "f16x2", "fp32", [](fd_context *c, bool a) { c->mode.conv_f16 = a; }},
        {"lvc_h8", "mfma", "valu", [](fd_context *c, bool a) { c->mode.lvc_h8_mfma = a; }},
        {"fallback", "graph", "host", [](fd_context *c, bool a) { c->host_fallback = !a; }},
        // training operator, frames path: gather = dx reads the forward-order frames; copy = a reordered copy first
        {"lvc_dx", "gather", "copy", [](fd_context *c, bool a) { c->lvc_dx_gather = a; }},
        {"mel", "pwg", "tacotron", [](fd_context *c, bool a) { c->mel_variant = a ? MEL_PWG : MEL_TACOTRON; }},
    };
    for (const auto &ch : choices) {
        if (k != ch.key) continue;
        if (v != ch.a && v != ch.b) FD_FAIL(h, FD_ERR_INVALID, "fd_set_option: %s expects %s|%s, got '%s'", key, ch.a, ch.b, value);
        ch.set(h, v == ch.a);
        return FD_OK;
    }
    const bool on = (v == "1" || v == "true" || v == "on");
    if (k == "fuse_final") { h->mode.fuse_final = on; return FD_OK; }
    if (k == "fuse_up") { h->mode.fuse_up = on; return FD_OK; }
    if (k == "fuse_advance") { h->mode.fuse_advance = on; return FD_OK; }
    if (k == "embed_cache") { h->embed_cache = on; return FD_OK; }
    if (k == "hoist") {
        if (v == "auto") h->hoist_mode = 1;
        else if (v == "on") h->hoist_mode = 2;
        else if (v == "off") h->hoist_mode = 0;
        else FD_FAIL(h, FD_ERR_INVALID, "fd_set_option: hoist expects auto|on|off, got '%s'", value);
        return FD_OK;
    }
    if (k == "graph") { h->use_graph = on; return FD_OK; }
    if (k == "defer_check") { h->defer_check = on; return FD_OK; }
    if (k == "t_bucket" || k == "graph_cache") {
        char *end = nullptr;
        const long n = strtol(value, &end, 10);
        if (end == value || *end != 0 || n < 0 || n > 65536 || (k == "graph_cache" && n < 1))
            FD_FAIL(h, FD_ERR_INVALID, "fd_set_option: %s expects an integer (t_bucket: frames, 0 = exact T; graph_cache: graphs kept, >= 1), got '%s'", key, value);
        if (k == "t_bucket") h->t_bucket = (int)n;
        else h->max_graphs = (int)n;
        return FD_OK;
    }
    if (k == "profile") { h->profile = (v == "events") ? 2 : (on ? 1 : 0); return FD_OK; }
    if (k == "taps") { h->mode.keep_taps = on; return FD_OK; }
    FD_FAIL(h, FD_ERR_INVALID, "fd_set_option: unknown option '%s'", key);
}

}  // extern "C"
