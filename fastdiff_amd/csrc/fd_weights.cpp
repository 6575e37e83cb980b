// fd_weights.cpp -- weight ingestion of libfastdiff_hip.so: fd_set_weight keeps host copies of the state_dict, fd_commit_weights folds
// weight norm, builds every operand pack of the tuned kernel set as a host image (fdg::pack_weights: the reference-layout weights of
// another architecture) and places that image on the device with one allocation and one copy.
#include <math.h>
#include <string.h>

#include "fd_host.h"
#include "fd_wpack.h"

// ------------------------------------------------------------------------------------------------
// expected state_dict (FastDiff_model.py:13-72; modules.py:116-125,141-187,257-318)
// ------------------------------------------------------------------------------------------------
struct ParamSpec { std::string name; std::vector<int64_t> dims; bool weight_norm; bool transposed_conv; bool linear; };

static const int KP_RES_IDX[6] = {1, 3, 6, 8, 11, 13};

// the state_dict of FastDiff(**cfg): names, shapes and registration facts (weight-normed Conv1d, plain ConvTranspose1d / Linear)
static std::vector<ParamSpec> param_specs(const fd_config &c)
{
    const int64_t C = c.inner_channels, COND = c.cond_channels, HID = c.kpnet_hidden_channels, KS = c.lvc_kernel_size, KK = c.kpnet_conv_size;
    const int64_t LAYERS = c.lvc_layers_each_block, E_IN = c.diffusion_step_embed_dim_in, E_MID = c.diffusion_step_embed_dim_mid, E_OUT = c.diffusion_step_embed_dim_out;
    std::vector<ParamSpec> s;
    s.push_back({"first_audio_conv", {C, 1, 7}, true, false, false});
    s.push_back({"fc_t1", {E_MID, E_IN}, false, false, true});
    s.push_back({"fc_t2", {E_OUT, E_MID}, false, false, true});
    for (int n = 0; n < c.n_upsample; ++n) {
        const std::string p = "lvc_blocks." + std::to_string(n);
        s.push_back({p + ".upsample", {C, C, 2 * (int64_t)c.upsample_ratios[n]}, false, true, false});
        s.push_back({p + ".kernel_predictor.input_conv.0", {HID, COND, 5}, true, false, false});
        for (int j = 0; j < 6; ++j)
            s.push_back({p + ".kernel_predictor.residual_conv." + std::to_string(KP_RES_IDX[j]), {HID, HID, KK}, true, false, false});
        s.push_back({p + ".kernel_predictor.kernel_conv", {LAYERS * C * 2 * C * KS, HID, KK}, true, false, false});
        s.push_back({p + ".kernel_predictor.bias_conv", {LAYERS * 2 * C, HID, KK}, true, false, false});
        s.push_back({p + ".fc_t", {COND, E_OUT}, false, false, true});
        for (int i = 0; i < LAYERS; ++i) s.push_back({p + ".convs." + std::to_string(i), {C, C, KS}, true, false, false});
        const std::string d = "downsample." + std::to_string(n);
        s.push_back({d + ".residual_dense", {C, C, 1}, true, false, false});
        for (int i = 0; i < 3; ++i) s.push_back({d + ".conv." + std::to_string(i), {C, C, 3}, true, false, false});
    }
    s.push_back({"final_conv.0", {c.audio_channels, C, 7}, true, false, false});
    return s;
}

static int64_t numel(const std::vector<int64_t> &d)
{
    int64_t n = 1;
    for (auto v : d) n *= v;
    return n;
}

// The shape a state_dict key must have (<parameter>.weight | weight_v | weight_g | bias), empty for a key the module does not have
static std::vector<int64_t> expected_dims(const std::vector<ParamSpec> &specs, const std::string &key)
{
    for (const auto &s : specs) {
        if (key.compare(0, s.name.size(), s.name) != 0 || key.size() <= s.name.size() || key[s.name.size()] != '.') continue;
        const std::string suffix = key.substr(s.name.size() + 1);
        if (suffix == "weight" || suffix == "weight_v") return s.dims;
        if (suffix == "weight_g") return {s.dims[0], 1, 1};
        if (suffix == "bias") return {s.transposed_conv ? s.dims[1] : s.dims[0]};
    }
    return {};
}

// ... and the check of one tensor against it, for fd_set_weight and fd_refresh_weights_device alike
static int check_dims(fd_handle h, const char *who, const std::vector<ParamSpec> &specs, const char *name, const int64_t *dims, int ndim)
{
    const std::vector<int64_t> expect = expected_dims(specs, name);
    if (expect.empty()) FD_FAIL(h, FD_ERR_INVALID, "%s: unexpected key '%s' (not in the FastDiff state_dict)", who, name);
    const std::vector<int64_t> got(dims, dims + ndim);
    if (got != expect) {
        std::string a, b;
        for (auto v : got) a += std::to_string(v) + ",";
        for (auto v : expect) b += std::to_string(v) + ",";
        FD_FAIL(h, FD_ERR_INVALID, "%s: size mismatch for %s: got [%s] expected [%s]", who, name, a.c_str(), b.c_str());
    }
    return FD_OK;
}

extern "C" int fd_set_weight(fd_handle h, const char *name, const float *host_data, const int64_t *dims, int ndim)
{
    if (!h || !name || !host_data || !dims || ndim <= 0 || ndim > 4) return FD_ERR_INVALID;
    const std::string key(name);
    const int rcd = check_dims(h, "fd_set_weight", param_specs(h->cfg), name, dims, ndim);
    if (rcd != FD_OK) return rcd;
    const std::vector<int64_t> got(dims, dims + ndim);
    auto &slot = h->raw[key];
    slot.first = got;
    slot.second.assign(host_data, host_data + numel(got));
    h->committed = false;
    return FD_OK;
}

namespace {

typedef FoldedParam Folded;
typedef std::map<std::string, Folded> FoldedSet;

// w = v * (g / ||v||), norm over everything but dim 0 (torch._weight_norm(v, g, 0)); plain weights pass through
int fold_param(fd_context *h, const ParamSpec &s, Folded &out)
{
    const auto itb = h->raw.find(s.name + ".bias");
    if (itb == h->raw.end()) FD_FAIL(h, FD_ERR_MISSING, "fd_commit_weights: missing tensor %s.bias", s.name.c_str());
    out.b = itb->second.second;
    const auto itw = h->raw.find(s.name + ".weight");
    const auto itv = h->raw.find(s.name + ".weight_v");
    const auto itg = h->raw.find(s.name + ".weight_g");
    if (itv != h->raw.end() && itg != h->raw.end()) {
        const std::vector<float> &v = itv->second.second, &g = itg->second.second;
        const int64_t cout = s.dims[0], per = numel(s.dims) / cout;
        out.w.resize(v.size());
        for (int64_t o = 0; o < cout; ++o) {
            double ss = 0.0;
            for (int64_t j = 0; j < per; ++j) ss += (double)v[o * per + j] * (double)v[o * per + j];
            const float scale = g[o] / (float)sqrt(ss);
            for (int64_t j = 0; j < per; ++j) out.w[o * per + j] = v[o * per + j] * scale;
        }
    } else if (itw != h->raw.end()) {
        out.w = itw->second.second;
    } else {
        FD_FAIL(h, FD_ERR_MISSING, "fd_commit_weights: missing tensor %s.weight (or weight_g/weight_v)", s.name.c_str());
    }
    return FD_OK;
}

using namespace fdp;      // the layouts: fd_wpack.h, shared with the device packer

// Conv weight [cout][cin][ks] -> MFMA A-operand pack [mt][s4][lane][4], kk = tap*cin + ci = 2*(4*s4+r) + (lane>>5)
std::vector<float> pack_A(const std::vector<float> &w, int cout, int cin, int ks)
{
    std::vector<float> p((size_t)(cout / 32) * (cin * ks / 8) * 256);
    for (size_t d = 0; d < p.size(); ++d) p[d] = w[pack_A_src((int)d, cin, ks)];
    return p;
}

// fp16 pieces of value(o, i) as [outer][piece][inner], and whether every value fits (the *_ok flag of the pack's kernel family)
struct Pieces { std::vector<uint16_t> h; bool ok = true; };
template <class F> Pieces pieces(int outer, int inner, F value)
{
    Pieces p;
    p.h.resize((size_t)outer * 2 * inner);
    for (int o = 0; o < outer; ++o)
        for (int i = 0; i < inner; ++i)
            if (!split_f16(value(o, i), p.h[((size_t)o * 2 + 0) * inner + i], p.h[((size_t)o * 2 + 1) * inner + i])) p.ok = false;
    return p;
}

// fp16 pieces of a conv weight [cout][cin][ks] (cout a multiple of 32) in 32x32x16 A-operand order:
// [mt = out/32][piece][kg][lane = out%32 + 32*g][8], k = tap*cin + in
Pieces pack_A_h2(const std::vector<float> &w, int cin, int ks, int cout = 32)
{
    return pieces(cout / 32, cin * ks / 16 * 512, [&](int mt, int i) { return w[pack_A_h2_src(mt, i, cin, ks)]; });
}

// The kernel_conv or bias_conv row behind packed column pp of the predictor GEMM: its weights [HID][3] and its bias.
struct GemmColumn { const float *w; float b; };
GemmColumn gemm_column(const Folded &kc, const Folded &bc, int pp)
{
    bool bias_conv;
    const int row = gemm_column_row(pp, &bias_conv);
    const Folded &f = bias_conv ? bc : kc;
    return {f.w.data() + (size_t)row * fd::HID * 3, f.b[row]};
}

// Every weight of the tuned kernel set (DevWeights) as a host image; sets the *_ok flags.  The pointer fields are written by upload().
void pack_tuned(const FoldedSet &f, DevWeights &w, WeightImage &img)
{
    auto F = [&](const std::string &name) -> const Folded & { return f.at(name); };
    auto add_conv = [&](const std::string &name, ConvW &cw) {
        img.add(cw.w, F(name).w);
        img.add(cw.b, F(name).b);
    };
    auto add_h2 = [&](const uint16_t *&dst, bool &ok, const Pieces &p) {
        img.add(dst, p.h);
        ok = ok && p.ok;
    };
    w.gemm_f16_ok = w.gemm_w_ok = w.lvc_f16_ok = w.dblock_f16_ok = w.convt_f16_ok = w.kpf_f16_ok = true;
    add_conv("first_audio_conv", w.first);
    add_conv("final_conv.0", w.final_);
    {   // the same weights in the order the last LVC layer holds its outputs: channel = 16 mt + 4 hi + (r & 3) + 8 (r >> 2)
        const std::vector<float> &fw = F("final_conv.0").w;
        std::vector<float> ff(4 * 8 * 8, 0.0f);
        for (int d = 0; d < 4 * 8 * 8; ++d)
            if (final_fuse_src(d) >= 0) ff[d] = fw[final_fuse_src(d)];
        img.add(w.final_fuse, ff);
    }
    // embed MLP, transposed
    auto transpose = [](const std::vector<float> &m, int rows, int cols) {
        std::vector<float> t((size_t)rows * cols);
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < cols; ++c) t[(size_t)c * rows + r] = m[(size_t)r * cols + c];
        return t;
    };
    img.add(w.fc_t1_T, transpose(F("fc_t1").w, fd::E_MID, fd::E_IN));
    img.add(w.fc_t1_b, F("fc_t1").b);
    img.add(w.fc_t2_T, transpose(F("fc_t2").w, fd::E_OUT, fd::E_MID));
    img.add(w.fc_t2_b, F("fc_t2").b);
    {   // frequency table of calc_diffusion_step_embedding (util.py:425-427): fp32 product, fp32 exp
        std::vector<float> table(64);
        const float cst = (float)(-(log(10000.0) / 63.0));
        for (int j = 0; j < 64; ++j) {
            volatile float arg = (float)j * cst;
            table[j] = expf(arg);
        }
        img.add(w.embed_table, table);
    }
    for (int n = 0; n < fd::NBLK; ++n) {
        const std::string p = "lvc_blocks." + std::to_string(n), d = "downsample." + std::to_string(n);
        add_conv(d + ".residual_dense", w.down[n].res);
        for (int i = 0; i < 3; ++i) {
            add_conv(d + ".conv." + std::to_string(i), w.down[n].conv[i]);
            img.add(w.down_pack[n][i], pack_A(F(d + ".conv." + std::to_string(i)).w, fd::C, fd::C, 3));
        }
        img.add(w.down_pack[n][3], pack_A(F(d + ".residual_dense").w, fd::C, fd::C, 1));
        for (int i = 0; i < 4; ++i)      // the same four matrices as fp16 pieces (conv 0..2: K = 96, residual 1x1: K = 32)
            add_h2(w.down_h2[n][i], w.dblock_f16_ok, pack_A_h2(F(i < 3 ? d + ".conv." + std::to_string(i) : d + ".residual_dense").w, fd::C, i < 3 ? 3 : 1));
        add_conv(p + ".fc_t", w.blk[n].fc_t);
        img.add(w.fc_t_T[n], transpose(F(p + ".fc_t").w, fd::COND, fd::E_OUT));
        add_conv(p + ".upsample", w.blk[n].up);
        {   // ConvTranspose1d weight [in][out][2r] -> per-phase MFMA A operands [ph][s4][lane][4], kk = sel*32 + i
            const int r = fd::ratio(n);
            const std::vector<float> &uw = F(p + ".upsample").w;
            std::vector<float> up((size_t)r * 8 * 256);
            for (size_t d = 0; d < up.size(); ++d) up[d] = uw[up_pack_src((int)d, r)];
            img.add(w.up_pack[n], up);
            // the same per-phase slices as fp16 pieces: [ph][piece][4 kg][64 lane = out + 32*g][8], k = 16*kg + 8*g + e = sel*32 + i
            add_h2(w.up_h2[n], w.convt_f16_ok, pieces(r, 4 * 512, [&](int ph, int i) { return uw[up_h2_src(ph, i, r)]; }));
        }
        add_conv(p + ".kernel_predictor.input_conv.0", w.blk[n].kp_in);
        img.add(w.kp_in_pack[n], pack_A(F(p + ".kernel_predictor.input_conv.0").w, fd::HID, fd::COND, 5));
        add_h2(w.kp_in_h2[n], w.kpf_f16_ok, pack_A_h2(F(p + ".kernel_predictor.input_conv.0").w, fd::COND, 5, fd::HID));
        for (int j = 0; j < 6; ++j) {
            const std::string nm = p + ".kernel_predictor.residual_conv." + std::to_string(KP_RES_IDX[j]);
            add_conv(nm, w.blk[n].kp_res[j]);
            img.add(w.kp_res_pack[n][j], pack_A(F(nm).w, fd::HID, fd::HID, 3));
            add_h2(w.kp_res_h2[n][j], w.kpf_f16_ok, pack_A_h2(F(nm).w, fd::HID, 3, fd::HID));
        }
        add_conv(p + ".kernel_predictor.kernel_conv", w.blk[n].kc);
        add_conv(p + ".kernel_predictor.bias_conv", w.blk[n].bc);
        for (int i = 0; i < fd::LAYERS; ++i) {
            const std::vector<float> &cw = F(p + ".convs." + std::to_string(i)).w;
            add_conv(p + ".convs." + std::to_string(i), w.blk[n].convs[i]);
            img.add(w.lvc_conv_pack[n][i], pack_A(cw, fd::C, fd::C, 3));
            if (n == 0)      // hop 8: 16x16x32 tiles [rt][tap][piece][64 lane][8]: lane = out%16 + 16*g holds input channels 8g .. 8g+7 of one tap
                add_h2(w.lvc_conv_h16[i], w.lvc_f16_ok, pieces(2 * 3, 512, [&](int rt_tap, int idx) { return cw[lvc_h16_src(rt_tap, idx)]; }));
            add_h2(w.lvc_conv_h2[n][i], w.lvc_f16_ok, pack_A_h2(cw, fd::C, 3));
        }
        // the predictor GEMM's B operands: one column per packed-record position pp, kk = tap*64 + channel
        std::vector<GemmColumn> col(fd::KREC);
        for (int pp = 0; pp < fd::KREC; ++pp)
            col[pp] = gemm_column(F(p + ".kernel_predictor.kernel_conv"), F(p + ".kernel_predictor.bias_conv"), pp);
        {   // fp32: [ptile][24 s4][lane][4], kk = 2*(4*s4+r) + (lane>>5)
            std::vector<float> gp((size_t)(fd::KREC / 32) * 24 * 256), gb(fd::KREC);
            for (int pt = 0; pt < fd::KREC / 32; ++pt)
                for (int d = 0; d < 24 * 256; ++d) {
                    const TilePos q = gemm_pack_pos(d);
                    gp[(size_t)pt * 24 * 256 + d] = col[pt * 32 + q.col].w[q.widx];
                }
            for (int pp = 0; pp < fd::KREC; ++pp) gb[pp] = col[pp].b;
            img.add(w.gemm_pack[n], gp);
            img.add(w.gemm_bias[n], gb);
        }
        // fp16x2 form, B operand of v_mfma_f32_32x32x16_f16: [ptile][piece][12 kg][lane = col + 32*g][8], k = tap*64 + channel
        add_h2(w.gemm_h2_pack[n], w.gemm_f16_ok, pieces(fd::KREC / 32, 12 * 512, [&](int pt, int i) {
                   const TilePos q = gemm_h2_pos(i);
                   return col[pt * 32 + q.col].w[q.widx];
               }));
        // Winograd F(2,3) over the frame axis (fd_wpack.h: gemm_w_value): B operand [ptile][piece][16 kg][lane = col + 32*g][8], k = 64 j + channel
        add_h2(w.gemm_w_pack[n], w.gemm_w_ok, pieces(fd::KREC / 32, 16 * 512, [&](int pt, int i) {
                   return gemm_w_value(i, [&](int c) { return col[pt * 32 + c].w; });
               }));
    }
    std::vector<int> perm(fd::KW);
    for (int layer = 0; layer < fd::LAYERS; ++layer)
        for (int in = 0; in < fd::C; ++in)
            for (int out = 0; out < 2 * fd::C; ++out)
                for (int tap = 0; tap < 3; ++tap)
                    perm[((layer * fd::C + in) * 2 * fd::C + out) * 3 + tap] = fd::kernel_index(layer, in, out, tap);
    img.add(w.kc_perm, perm);
    std::vector<int> bperm(fd::KB);
    for (int layer = 0; layer < fd::LAYERS; ++layer)
        for (int out = 0; out < 2 * fd::C; ++out) bperm[layer * 64 + out] = fd::bias_index(layer, out) - fd::KW;
    img.add(w.bc_perm, bperm);
}

// One device allocation for the whole image and one copy, then the pointer fields.  A failure leaves nothing allocated and no field
// written.
int upload(fd_context *h, const WeightImage &img)
{
    void *d = nullptr;
    FD_HIP(h, hipMalloc(&d, img.bytes.size()));
    const hipError_t e = hipMemcpy(d, img.bytes.data(), img.bytes.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        FD_FAIL(h, FD_ERR_HIP, "fd_commit_weights: weight upload failed: %s", hipGetErrorString(e));
    }
    h->weight_arena = d;
    h->weight_bytes = img.bytes.size();
    for (const auto &fl : img.fields) *fl.first = static_cast<const char *>(d) + fl.second;
    return FD_OK;
}

}  // namespace

extern "C" int fd_commit_weights(fd_handle h)
{
    if (!h) return FD_ERR_INVALID;
    FD_HIP(h, hipSetDevice(h->device));
    {
        const int rcs = fd_settle(h);      // a pending host check would otherwise run its call again on the NEW weights
        if (rcs != FD_OK) return rcs;
    }
    h->embed_valid = false;
    FD_HIP(h, hipDeviceSynchronize());
    h->committed = false;            // until the new set is complete: a failed re-commit must not leave the old flag over freed weights
    if (h->weight_arena) (void)hipFree(h->weight_arena);
    h->weight_arena = nullptr;
    h->weight_bytes = 0;
    h->refresh_pending = false;      // (the device is idle: a refresh's flags are moot, the new set brings its own)
    h->w = DevWeights();
    drop_graph(h);

    FoldedSet f;
    for (const auto &s : param_specs(h->cfg)) {
        int rc = fold_param(h, s, f[s.name]);
        if (rc != FD_OK) return rc;
    }
    WeightImage img;
    if (h->gen) {      // another architecture than base.yaml's: folded reference-layout weights, no operand packing
        int rc = fdg::pack_weights(h, f, img);
        if (rc == FD_OK) rc = upload(h, img);
        if (rc == FD_OK) h->committed = true;
        return rc;
    }
    DevWeights w;
    pack_tuned(f, w, img);
    const int rc = upload(h, img);
    if (rc != FD_OK) return rc;
    for (int n = 0; n < fd::NBLK; ++n) w.fc_t_b[n] = w.blk[n].fc_t.b;      // the same bias: an alias, not a second copy
    h->w = w;
    h->raw.clear();     // host copies are no longer needed
    h->committed = true;
    return FD_OK;
}

// ------------------------------------------------------------------------------------------------
// the same packs rebuilt on the device, in place, from live parameter tensors (fd_kernels_wpack.hip)
// ------------------------------------------------------------------------------------------------
namespace {

struct LiveParam { const float *w = nullptr, *v = nullptr, *g = nullptr, *b = nullptr; };

// The work lists of one refresh: what pack_tuned does, restated as jobs over the arena's own slots.  Weight norm folds into the
// reference-layout slot of its parameter (ConvW::w -- the arena already holds every folded weight once, so those slots are the folded
// staging and nothing is held twice); `live` jobs read the caller's tensors, `packs` jobs the slots, so they run behind them.
struct RefreshJobs {
    std::vector<fdk::FoldJob> fold;
    std::vector<fdk::PackJob> live, packs;
    fdk::GemmJobs gemm;
    int fold_blocks = 0, live_blocks = 0, pack_blocks = 0;

    void add_fold(const float *v, const float *g, const float *dst, int rows, int per)
    {
        const int rpb = fdk::wpack_fold_rows(per);
        fold.push_back({v, g, const_cast<float *>(dst), rows, per, rpb, fold_blocks});
        fold_blocks += (rows + rpb - 1) / rpb;
    }
    void add(std::vector<fdk::PackJob> &list, int &blocks, int kind, const float *src, const void *dst, int n, int p0 = 0, int p1 = 0,
             int inner = 1, int flag = 0)
    {
        list.push_back({src, const_cast<void *>(dst), kind, n, p0, p1, inner, flag, blocks, 0});
        const int units = kind >= fdk::WP_A_H2 ? n / 8 : (n + 3) / 4;
        blocks += (units + 255) / 256;
    }
    void copy(const float *src, const float *dst, int64_t n) { add(live, live_blocks, fdk::WP_COPY, src, dst, (int)n); }
    void pack(int kind, const float *src, const void *dst, int n, int p0 = 0, int p1 = 0, int inner = 1, int flag = 0)
    {
        add(packs, pack_blocks, kind, src, dst, n, p0, p1, inner, flag);
    }
    void pack_A(const float *src, const float *dst, int cout, int cin, int ks) { pack(fdk::WP_PACK_A, src, dst, cout / 32 * (cin * ks / 8) * 256, cin, ks); }
    void pack_A_h2(const float *src, const uint16_t *dst, int cout, int cin, int ks, int flag)
    {
        const int inner = cin * ks / 16 * 512;
        pack(fdk::WP_A_H2, src, dst, cout / 32 * inner, cin, ks, inner, flag);
    }
};

int build_refresh_jobs(fd_context *h, const std::vector<ParamSpec> &specs, const std::map<std::string, LiveParam> &live, RefreshJobs &J)
{
    const DevWeights &w = h->w;
    std::map<std::string, const ParamSpec *> spec;
    for (const auto &s : specs) spec[s.name] = &s;
    // a parameter into its reference-layout slot: the bias copied, the weight folded or copied
    auto conv = [&](const std::string &name, const ConvW &cw) {
        const ParamSpec &s = *spec.at(name);
        const LiveParam &p = live.at(name);
        const int64_t nw = numel(s.dims);
        J.copy(p.b, cw.b, s.transposed_conv ? s.dims[1] : s.dims[0]);
        if (p.v) J.add_fold(p.v, p.g, cw.w, (int)s.dims[0], (int)(nw / s.dims[0]));
        else J.copy(p.w, cw.w, nw);
    };
    conv("first_audio_conv", w.first);
    conv("final_conv.0", w.final_);
    J.pack(fdk::WP_FINAL_FUSE, w.final_.w, w.final_fuse, 4 * 8 * 8);
    // the embed MLP has no reference-layout slot: transposed straight from the caller's tensors
    const struct { const char *name; const float *T, *b; int rows, cols; } mlp[2] = {{"fc_t1", w.fc_t1_T, w.fc_t1_b, fd::E_MID, fd::E_IN},
                                                                                   {"fc_t2", w.fc_t2_T, w.fc_t2_b, fd::E_OUT, fd::E_MID}};
    for (const auto &m : mlp) {
        const LiveParam &p = live.at(m.name);
        if (p.v) FD_FAIL(h, FD_ERR_UNSUPPORTED, "fd_refresh_weights_device: %s is weight-normed (a Linear of the reference is not): use fd_set_weight + fd_commit_weights", m.name);
        J.add(J.live, J.live_blocks, fdk::WP_TRANSPOSE, p.w, m.T, m.rows * m.cols, m.rows, m.cols);
        J.copy(p.b, m.b, m.rows);
    }
    for (int n = 0; n < fd::NBLK; ++n) {
        const std::string p = "lvc_blocks." + std::to_string(n), d = "downsample." + std::to_string(n);
        conv(d + ".residual_dense", w.down[n].res);
        for (int i = 0; i < 3; ++i) conv(d + ".conv." + std::to_string(i), w.down[n].conv[i]);
        for (int i = 0; i < 4; ++i) {      // conv 0..2: K = 96, residual 1x1: K = 32
            const float *src = i < 3 ? w.down[n].conv[i].w : w.down[n].res.w;
            J.pack_A(src, w.down_pack[n][i], fd::C, fd::C, i < 3 ? 3 : 1);
            J.pack_A_h2(src, w.down_h2[n][i], fd::C, fd::C, i < 3 ? 3 : 1, OK_DBLOCK);
        }
        conv(p + ".fc_t", w.blk[n].fc_t);
        J.pack(fdk::WP_TRANSPOSE, w.blk[n].fc_t.w, w.fc_t_T[n], fd::COND * fd::E_OUT, fd::COND, fd::E_OUT);
        conv(p + ".upsample", w.blk[n].up);
        const int r = fd::ratio(n);
        J.pack(fdk::WP_UP_PACK, w.blk[n].up.w, w.up_pack[n], r * 8 * 256, r);
        J.pack(fdk::WP_UP_H2, w.blk[n].up.w, w.up_h2[n], r * 4 * 512, r, 0, 4 * 512, OK_CONVT);
        conv(p + ".kernel_predictor.input_conv.0", w.blk[n].kp_in);
        J.pack_A(w.blk[n].kp_in.w, w.kp_in_pack[n], fd::HID, fd::COND, 5);
        J.pack_A_h2(w.blk[n].kp_in.w, w.kp_in_h2[n], fd::HID, fd::COND, 5, OK_KPF);
        for (int j = 0; j < 6; ++j) {
            conv(p + ".kernel_predictor.residual_conv." + std::to_string(KP_RES_IDX[j]), w.blk[n].kp_res[j]);
            J.pack_A(w.blk[n].kp_res[j].w, w.kp_res_pack[n][j], fd::HID, fd::HID, 3);
            J.pack_A_h2(w.blk[n].kp_res[j].w, w.kp_res_h2[n][j], fd::HID, fd::HID, 3, OK_KPF);
        }
        conv(p + ".kernel_predictor.kernel_conv", w.blk[n].kc);
        conv(p + ".kernel_predictor.bias_conv", w.blk[n].bc);
        for (int i = 0; i < fd::LAYERS; ++i) {
            const float *cw = w.blk[n].convs[i].w;
            conv(p + ".convs." + std::to_string(i), w.blk[n].convs[i]);
            J.pack_A(cw, w.lvc_conv_pack[n][i], fd::C, fd::C, 3);
            if (n == 0) J.pack(fdk::WP_H16, cw, w.lvc_conv_h16[i], 2 * 3 * 512, 0, 0, 512, OK_LVC);
            J.pack_A_h2(cw, w.lvc_conv_h2[n][i], fd::C, fd::C, 3, OK_LVC);
        }
        J.gemm.blk[n] = {w.blk[n].kc.w, w.blk[n].kc.b, w.blk[n].bc.w, w.blk[n].bc.b, const_cast<float *>(w.gemm_pack[n]),
                         const_cast<float *>(w.gemm_bias[n]), const_cast<uint16_t *>(w.gemm_h2_pack[n]), const_cast<uint16_t *>(w.gemm_w_pack[n])};
    }
    return FD_OK;
}

unsigned ok_mask(const DevWeights &w)
{
    return (w.gemm_f16_ok ? OK_GEMM : 0) | (w.gemm_w_ok ? OK_GEMM_W : 0) | (w.lvc_f16_ok ? OK_LVC : 0) | (w.dblock_f16_ok ? OK_DBLOCK : 0) |
           (w.convt_f16_ok ? OK_CONVT : 0) | (w.kpf_f16_ok ? OK_KPF : 0);
}

}  // namespace

extern "C" int fd_refresh_weights_device(fd_handle h, const fd_weight_ref *items, int n, void *stream_)
{
    if (!h || !items || n <= 0) return FD_ERR_INVALID;
    hipStream_t stream = (hipStream_t)stream_;
    if (h->gen)
        FD_FAIL(h, FD_ERR_UNSUPPORTED, "fd_refresh_weights_device: the packs of base.yaml's architecture only; this handle runs another "
                                       "configuration (fd_set_weight + fd_commit_weights)");
    if (!h->committed || !h->weight_arena)
        FD_FAIL(h, FD_ERR_INVALID, "fd_refresh_weights_device: no committed weights to refresh (fd_commit_weights lays the arena out; call it once first)");
    // every tensor against the state_dict, before anything is written
    const std::vector<ParamSpec> specs = param_specs(h->cfg);
    std::map<std::string, LiveParam> live;
    for (int i = 0; i < n; ++i) {
        const fd_weight_ref &it = items[i];
        if (!it.name || !it.data || !it.dims || it.ndim <= 0 || it.ndim > 4) FD_FAIL(h, FD_ERR_INVALID, "fd_refresh_weights_device: item %d is incomplete", i);
        const int rc = check_dims(h, "fd_refresh_weights_device", specs, it.name, it.dims, it.ndim);
        if (rc != FD_OK) return rc;
        const std::string key(it.name);
        const size_t dot = key.rfind('.');
        LiveParam &p = live[key.substr(0, dot)];
        const std::string suffix = key.substr(dot + 1);
        (suffix == "weight" ? p.w : suffix == "weight_v" ? p.v : suffix == "weight_g" ? p.g : p.b) = it.data;
    }
    for (const auto &s : specs) {
        const LiveParam &p = live[s.name];
        if (!p.b) FD_FAIL(h, FD_ERR_INVALID, "fd_refresh_weights_device: missing tensor %s.bias", s.name.c_str());
        if (!(p.v && p.g) && !p.w) FD_FAIL(h, FD_ERR_INVALID, "fd_refresh_weights_device: missing tensor %s.weight (or weight_g/weight_v)", s.name.c_str());
        if (!(p.v && p.g)) live[s.name].v = live[s.name].g = nullptr;      // like the host fold: weight_v and weight_g together, else weight
    }
    RefreshJobs J;
    int rc = build_refresh_jobs(h, specs, live, J);
    if (rc != FD_OK) return rc;

    FD_HIP(h, hipSetDevice(h->device));
    if ((rc = fd_settle(h)) != FD_OK) return rc;      // a pending host check would otherwise run its call again on the NEW weights
    if ((rc = fd_follow_stream(h, stream)) != FD_OK) return rc;
    // device memory of the lists: [256 bytes: the word of out-of-range families][fold][live][packs].  The same size at every call.
    const size_t fold_b = J.fold.size() * sizeof(fdk::FoldJob), live_b = J.live.size() * sizeof(fdk::PackJob), pack_b = J.packs.size() * sizeof(fdk::PackJob);
    const size_t lists_b = fold_b + live_b + pack_b, need = 256 + lists_b;
    if (h->refresh_dev_bytes < need) {      // the first refresh (outside any capture); never again
        if (h->refresh_dev) {
            FD_HIP(h, hipDeviceSynchronize());
            (void)hipFree(h->refresh_dev);
            h->refresh_dev = nullptr;
            h->refresh_dev_bytes = 0;
        }
        FD_HIP(h, hipMalloc(&h->refresh_dev, need));
        h->refresh_dev_bytes = need;
    }
    if (!h->refresh_bad) FD_HIP(h, hipHostMalloc(reinterpret_cast<void **>(&h->refresh_bad), sizeof(unsigned), hipHostMallocDefault));
    if (!h->refresh_done) FD_HIP(h, hipEventCreateWithFlags(&h->refresh_done, hipEventDisableTiming));
    char *dev = static_cast<char *>(h->refresh_dev);
    unsigned *bad = reinterpret_cast<unsigned *>(dev);
    fd_context::StageSlot *sl = nullptr;
    if ((rc = fd_stage_acquire(h, lists_b, &sl)) != FD_OK) return rc;
    memcpy(sl->host, J.fold.data(), fold_b);
    memcpy(sl->host + fold_b, J.live.data(), live_b);
    memcpy(sl->host + fold_b + live_b, J.packs.data(), pack_b);
    FD_HIP(h, hipMemsetAsync(bad, 0, sizeof(unsigned), stream));
    FD_HIP(h, hipMemcpyAsync(dev + 256, sl->host, lists_b, hipMemcpyHostToDevice, stream));
    if ((rc = fd_stage_commit(h, sl, stream)) != FD_OK) return rc;

    h->embed_valid = false;      // the cached embedding rows are the old weights'
    fdk::Launch L = {h, stream, false};
    hipError_t e = fdk::wpack_fold(L, reinterpret_cast<const fdk::FoldJob *>(dev + 256), (int)J.fold.size(), J.fold_blocks);
    if (e == hipSuccess) e = fdk::wpack_gather(L, reinterpret_cast<const fdk::PackJob *>(dev + 256 + fold_b), (int)J.live.size(), J.live_blocks, bad);
    if (e == hipSuccess)
        e = fdk::wpack_gather(L, reinterpret_cast<const fdk::PackJob *>(dev + 256 + fold_b + live_b), (int)J.packs.size(), J.pack_blocks, bad);
    if (e == hipSuccess) e = fdk::wpack_gemm(L, J.gemm, bad);
    if (e != hipSuccess) FD_FAIL(h, FD_ERR_HIP, "fd_refresh_weights_device: kernel launch failed: %s", hipGetErrorString(e));
    FD_HIP(h, hipMemcpyAsync(h->refresh_bad, bad, sizeof(unsigned), hipMemcpyDeviceToHost, stream));
    FD_HIP(h, hipEventRecord(h->refresh_done, stream));
    h->refresh_pending = true;
    ++h->n_refreshes;
    return fd_mark_tail(h, stream);
}

// The flags of the last refresh, once: a changed flag changes which kernels a step launches, which the captured graphs have baked in.
extern "C" int fd_settle_refresh(fd_handle h)
{
    if (!h->refresh_pending) return FD_OK;
    FD_HIP(h, hipEventSynchronize(h->refresh_done));
    h->refresh_pending = false;
    const unsigned ok = OK_ALL & ~*h->refresh_bad;
    if (ok == ok_mask(h->w)) return FD_OK;
    const int rc = fd_settle(h);
    if (rc != FD_OK) return rc;
    FD_HIP(h, hipDeviceSynchronize());
    h->w.gemm_f16_ok = ok & OK_GEMM; h->w.gemm_w_ok = ok & OK_GEMM_W; h->w.lvc_f16_ok = ok & OK_LVC;
    h->w.dblock_f16_ok = ok & OK_DBLOCK; h->w.convt_f16_ok = ok & OK_CONVT; h->w.kpf_f16_ok = ok & OK_KPF;
    drop_graph(h);
    ++h->n_refresh_graph_drops;
    return FD_OK;
}

extern "C" int fd_get_weight_image(fd_handle h, void *host_buf, size_t *nbytes)
{
    if (!h || !nbytes) return FD_ERR_INVALID;
    if (!h->committed || !h->weight_arena) FD_FAIL(h, FD_ERR_STATE, "fd_get_weight_image: weights not committed");
    if (!host_buf) { *nbytes = h->weight_bytes; return FD_OK; }
    if (*nbytes < h->weight_bytes) FD_FAIL(h, FD_ERR_INVALID, "fd_get_weight_image: buffer of %zu bytes, the image has %zu", *nbytes, h->weight_bytes);
    FD_HIP(h, hipSetDevice(h->device));
    FD_HIP(h, hipDeviceSynchronize());
    FD_HIP(h, hipMemcpy(host_buf, h->weight_arena, h->weight_bytes, hipMemcpyDeviceToHost));
    *nbytes = h->weight_bytes;
    return FD_OK;
}

extern "C" int fd_get_weight_flags(fd_handle h, unsigned *ok)
{
    if (!h || !ok) return FD_ERR_INVALID;
    if (!h->committed) FD_FAIL(h, FD_ERR_STATE, "fd_get_weight_flags: weights not committed");
    if (h->gen) FD_FAIL(h, FD_ERR_UNSUPPORTED, "fd_get_weight_flags: the flags of the tuned kernel set; this handle runs another configuration");
    FD_HIP(h, hipSetDevice(h->device));
    const int rc = fd_settle_refresh(h);
    if (rc != FD_OK) return rc;
    *ok = ok_mask(h->w);
    return FD_OK;
}

extern "C" int fd_pack_source(const char *pack, int p0, int p1, int pos)
{
    if (!pack || pos < 0) return FD_ERR_INVALID;
    const std::string k(pack);
    if (k == "pack_a") return pack_A_src(pos, p0, p1);
    if (k == "a_h2") { const int inner = p0 * p1 / 16 * 512; return pack_A_h2_src(pos / inner, pos % inner, p0, p1); }
    if (k == "up") return up_pack_src(pos, p0);
    if (k == "up_h2") return up_h2_src(pos / 2048, pos % 2048, p0);
    if (k == "h16") return lvc_h16_src(pos / 512, pos % 512);
    if (k == "final_fuse") return final_fuse_src(pos) < 0 ? fd::C * 7 : final_fuse_src(pos);
    if (k == "gemm_row") { bool b; const int row = gemm_column_row(pos, &b); return b ? fd::KW + row : row; }
    if (k == "gemm") { const TilePos q = gemm_pack_pos(pos); return q.col * fd::HID * 3 + q.widx; }
    if (k == "gemm_h2") { const TilePos q = gemm_h2_pos(pos); return q.col * fd::HID * 3 + q.widx; }
    return FD_ERR_INVALID;
}
