// fd_weights.cpp -- weight ingestion of libfastdiff_hip.so: fd_set_weight keeps host copies of the state_dict, fd_commit_weights folds
// weight norm, builds every operand pack of the tuned kernel set as a host image (fdg::pack_weights: the reference-layout weights of
// another architecture) and places that image on the device with one allocation and one copy.
#include <math.h>
#include <string.h>

#include "fd_host.h"

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

extern "C" int fd_set_weight(fd_handle h, const char *name, const float *host_data, const int64_t *dims, int ndim)
{
    if (!h || !name || !host_data || !dims || ndim <= 0 || ndim > 4) return FD_ERR_INVALID;
    const std::string key(name);
    // find the owning parameter and the expected shape of this tensor
    const std::vector<ParamSpec> specs = param_specs(h->cfg);
    std::vector<int64_t> expect;
    for (const auto &s : specs) {
        if (key.compare(0, s.name.size(), s.name) != 0 || key.size() <= s.name.size() || key[s.name.size()] != '.') continue;
        const std::string suffix = key.substr(s.name.size() + 1);
        if (suffix == "weight" || suffix == "weight_v") expect = s.dims;
        else if (suffix == "weight_g") { expect = {s.dims[0], 1, 1}; }
        else if (suffix == "bias") expect = {s.transposed_conv ? s.dims[1] : s.dims[0]};
        else continue;
        break;
    }
    if (expect.empty()) FD_FAIL(h, FD_ERR_INVALID, "fd_set_weight: unexpected key '%s' (not in the FastDiff state_dict)", name);
    std::vector<int64_t> got(dims, dims + ndim);
    if (got != expect) {
        std::string a, b;
        for (auto v : got) a += std::to_string(v) + ",";
        for (auto v : expect) b += std::to_string(v) + ",";
        FD_FAIL(h, FD_ERR_INVALID, "fd_set_weight: size mismatch for %s: got [%s] expected [%s]", name, a.c_str(), b.c_str());
    }
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

// Conv weight [cout][cin][ks] -> MFMA A-operand pack [mt][s4][lane][4], kk = tap*cin + ci = 2*(4*s4+r) + (lane>>5)
std::vector<float> pack_A(const std::vector<float> &w, int cout, int cin, int ks)
{
    const int ns4 = cin * ks / 8, nmt = cout / 32;
    std::vector<float> p((size_t)nmt * ns4 * 256);
    for (int mt = 0; mt < nmt; ++mt)
        for (int s4 = 0; s4 < ns4; ++s4)
            for (int lane = 0; lane < 64; ++lane)
                for (int r = 0; r < 4; ++r) {
                    const int o = mt * 32 + (lane & 31), kk = 2 * (4 * s4 + r) + (lane >> 5);
                    const int tap = kk / cin, ci = kk % cin;
                    p[(((size_t)mt * ns4 + s4) * 64 + lane) * 4 + r] = w[((size_t)o * cin + ci) * ks + tap];
                }
    return p;
}

// IEEE binary16 <-> binary32 on the host (round to nearest even, subnormals kept): the weight pieces of the fp16x2 GEMM.
uint16_t f16_from_f32(float x)
{
    uint32_t u;
    memcpy(&u, &x, 4);
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
    u &= 0x7FFFFFFFu;
    if (u > 0x7F800000u) return sign | 0x7E00u;                  // NaN
    if (u >= 0x477FF000u) return sign | 0x7C00u;                 // >= 65520 rounds to infinity
    if (u < 0x38800000u) {                                       // below 2^-14: subnormal, a multiple of 2^-24
        float ax;
        memcpy(&ax, &u, 4);
        return sign | (uint16_t)lrintf(ax * 16777216.0f);        // current rounding mode = nearest even; 1024 = smallest normal
    }
    uint32_t hbits = (((u >> 23) - 112u) << 10) | ((u & 0x7FFFFFu) >> 13);
    const uint32_t rem = u & 0x1FFFu;
    if (rem > 0x1000u || (rem == 0x1000u && (hbits & 1u))) ++hbits;   // a carry into the exponent is the correct result
    return sign | (uint16_t)hbits;
}
float f32_from_f16(uint16_t hb)
{
    const uint32_t sign = (uint32_t)(hb & 0x8000u) << 16, exp = (hb >> 10) & 0x1Fu, man = hb & 0x3FFu;
    float v;
    if (exp == 0) v = (float)man * (1.0f / 16777216.0f);
    else if (exp == 31) { const uint32_t u = 0x7F800000u | (man << 13); memcpy(&v, &u, 4); }
    else { const uint32_t u = ((exp + 112u) << 23) | (man << 13); memcpy(&v, &u, 4); }
    uint32_t u;
    memcpy(&u, &v, 4);
    u |= sign;
    memcpy(&v, &u, 4);
    return v;
}

// The fp16x2 form of a weight: v = hi + 2^-11 lo, hi = fp16(v), lo = fp16((v - hi) * 2^11).  False when v does not fit the range the
// fp16-pipe kernels accept (|v| < 32768).
bool split_f16(float v, uint16_t &hi, uint16_t &lo)
{
    hi = f16_from_f32(v);
    lo = f16_from_f32((v - f32_from_f16(hi)) * 2048.0f);
    return fabsf(v) < 32768.0f;
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

// Position i of a [kg][64 lane][8 e] run of 32x32x16 fp16 operands: lane = row + 32*g holds the 8 consecutive k = 16*kg + 8*g + e.
struct Op16 { int row, k; };
inline Op16 op16(int i) { return {(i >> 3) & 31, 16 * (i >> 9) + 8 * ((i >> 8) & 1) + (i & 7)}; }

// fp16 pieces of a conv weight [cout][cin][ks] (cout a multiple of 32) in 32x32x16 A-operand order:
// [mt = out/32][piece][kg][lane = out%32 + 32*g][8], k = tap*cin + in
Pieces pack_A_h2(const std::vector<float> &w, int cin, int ks, int cout = 32)
{
    return pieces(cout / 32, cin * ks / 16 * 512, [&](int mt, int i) {
        const Op16 q = op16(i);
        return w[((size_t)(mt * 32 + q.row) * cin + q.k % cin) * ks + q.k / cin];
    });
}

void unpack_kernel_index(int p, int &layer, int &in, int &out, int &tap)
{
    layer = p / fd::KLAYER;
    const int q = p % fd::KLAYER, e = q & 7, lane = (q >> 3) & 63, mk = q >> 9;
    const int mt = mk / 6, kg = mk % 6, kk = kg * 16 + 8 * (lane >> 5) + e, row = lane & 31;
    tap = kk / fd::C; in = kk % fd::C;
    out = 16 * mt + (row & 15) + 32 * (row >> 4);      // inverse of kernel_tile / kernel_row
}

// The kernel_conv or bias_conv row behind packed column pp of the predictor GEMM: its weights [HID][3] and its bias.
struct GemmColumn { const float *w; float b; };
GemmColumn gemm_column(const Folded &kc, const Folded &bc, int pp)
{
    if (pp < fd::KW) {
        int layer, in, out, tap;
        unpack_kernel_index(pp, layer, in, out, tap);
        const int row = ((layer * fd::C + in) * 2 * fd::C + out) * 3 + tap;   // [layers,in,out,k] view (modules.py:333-338)
        return {kc.w.data() + (size_t)row * fd::HID * 3, kc.b[row]};
    }
    // bias record [layer][mt][row]  ->  bias_conv row layer*64 + out (view [layers,out], modules.py:339-342)
    const int q = pp - fd::KW, layer = q >> 6, mt = (q >> 5) & 1, row = q & 31;
    const int brow = layer * 64 + 16 * mt + (row & 15) + 32 * (row >> 4);
    return {bc.w.data() + (size_t)brow * fd::HID * 3, bc.b[brow]};
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
        for (int part = 0; part < 4; ++part)
            for (int r = 0; r < 8; ++r)
                for (int k = 0; k < 7; ++k) ff[(part * 8 + r) * 8 + k] = fw[(16 * (part >> 1) + 4 * (part & 1) + (r & 3) + 8 * (r >> 2)) * 7 + k];
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
            const int r = fd::ratio(n), ks = 2 * r, pd = r / 2;
            const std::vector<float> &uw = F(p + ".upsample").w;
            // sel 0: the nearer input position (jA), sel 1: the one before it (jB = jA - 1, tap + r)
            auto tap = [&](int ph, int sel) { const int kA = (ph < pd) ? ph + pd : ph - pd; return sel ? kA + r : kA; };
            std::vector<float> up((size_t)r * 8 * 256);
            for (int ph = 0; ph < r; ++ph)
                for (int s4 = 0; s4 < 8; ++s4)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int q = 0; q < 4; ++q) {
                            const int kk = 2 * (4 * s4 + q) + (lane >> 5), i = kk & 31, o = lane & 31;
                            up[(((size_t)ph * 8 + s4) * 64 + lane) * 4 + q] = uw[((size_t)i * fd::C + o) * ks + tap(ph, kk >> 5)];
                        }
            img.add(w.up_pack[n], up);
            // the same per-phase slices as fp16 pieces: [ph][piece][4 kg][64 lane = out + 32*g][8], k = 16*kg + 8*g + e = sel*32 + i
            add_h2(w.up_h2[n], w.convt_f16_ok, pieces(r, 4 * 512, [&](int ph, int i) {
                       const Op16 q = op16(i);
                       return uw[((size_t)(q.k & 31) * fd::C + q.row) * ks + tap(ph, q.k >> 5)];
                   }));
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
                add_h2(w.lvc_conv_h16[i], w.lvc_f16_ok, pieces(2 * 3, 512, [&](int rt_tap, int idx) {
                           const int rt = rt_tap / 3, tap = rt_tap % 3, lane = idx >> 3, out = 16 * rt + (lane & 15), in = 8 * (lane >> 4) + (idx & 7);
                           return cw[((size_t)out * fd::C + in) * 3 + tap];
                       }));
            add_h2(w.lvc_conv_h2[n][i], w.lvc_f16_ok, pack_A_h2(cw, fd::C, 3));
        }
        // the predictor GEMM's B operands: one column per packed-record position pp, kk = tap*64 + channel
        std::vector<GemmColumn> col(fd::KREC);
        for (int pp = 0; pp < fd::KREC; ++pp)
            col[pp] = gemm_column(F(p + ".kernel_predictor.kernel_conv"), F(p + ".kernel_predictor.bias_conv"), pp);
        {   // fp32: [ptile][24 s4][lane][4], kk = 2*(4*s4+r) + (lane>>5)
            std::vector<float> gp((size_t)(fd::KREC / 32) * 24 * 256), gb(fd::KREC);
            for (int pt = 0; pt < fd::KREC / 32; ++pt)
                for (int lane = 0; lane < 64; ++lane)
                    for (int s4 = 0; s4 < 24; ++s4)
                        for (int r = 0; r < 4; ++r) {
                            const int kk = 2 * (4 * s4 + r) + (lane >> 5), tap = kk / fd::HID, c = kk % fd::HID;
                            gp[(((size_t)pt * 24 + s4) * 64 + lane) * 4 + r] = col[pt * 32 + (lane & 31)].w[c * 3 + tap];
                        }
            for (int pp = 0; pp < fd::KREC; ++pp) gb[pp] = col[pp].b;
            img.add(w.gemm_pack[n], gp);
            img.add(w.gemm_bias[n], gb);
        }
        // fp16x2 form, B operand of v_mfma_f32_32x32x16_f16: [ptile][piece][12 kg][lane = col + 32*g][8], k = tap*64 + channel
        add_h2(w.gemm_h2_pack[n], w.gemm_f16_ok, pieces(fd::KREC / 32, 12 * 512, [&](int pt, int i) {
                   const Op16 q = op16(i);
                   return col[pt * 32 + q.row].w[(q.k % fd::HID) * 3 + q.k / fd::HID];
               }));
        // Winograd F(2,3) over the frame axis (kernel_conv is a k = 3 convolution over frames, modules.py:315-318): per pair of
        // output frames  y[2p] = m0 + m1 + m2,  y[2p+1] = m1 - m2 + m3  with  m_j = V_j . u_j (K = 64 each),
        //   V0 = g0, V1 = (g0 + g1 + g2) / 2, V2 = (g0 - g1 + g2) / 2, V3 = -g2        (g_tap = the column's weights of that tap)
        //   u0 = h[2p-1] - h[2p+1], u1 = h[2p] + h[2p+1], u2 = h[2p+1] - h[2p], u3 = h[2p] - h[2p+2]   (k_h_wino)
        // B operand [ptile][piece][16 kg][lane = col + 32*g][8]: k = 64 j + channel
        add_h2(w.gemm_w_pack[n], w.gemm_w_ok, pieces(fd::KREC / 32, 16 * 512, [&](int pt, int i) {
                   const Op16 q = op16(i);
                   const int j = q.k >> 6, ch = q.k & 63;
                   const float *wrow = col[pt * 32 + q.row].w;
                   const double g0 = wrow[ch * 3 + 0], g1 = wrow[ch * 3 + 1], g2 = wrow[ch * 3 + 2];
                   return (float)(j == 0 ? g0 : (j == 1 ? 0.5 * (g0 + g1 + g2) : (j == 2 ? 0.5 * (g0 - g1 + g2) : -g2)));
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
