// gemm16_index_check.cpp -- the index arithmetic of k_kp_gemm_w<16> (fd_kernels_kp.hip: gw16_item) walked on the host: all 64 lanes x
// all registers of every item of an utterance of T frames, through the very lane maps the kernel uses (fd_kernels.h: gw16_*).
//
// Checked for T in {1, 31, 32, 33, 63, 64, 65, 864}:
//   * every A-operand read lies inside the item's 32 KB window and inside the image, and is the 16-byte slot that k_h_wino wrote for
//     (pair row, sub-row j, piece, K group);
//   * every B-operand read lies inside the block's gemm_w_pack and is the position fd_wpack.h's op16 gives (column, K group);
//   * every (frame, position) of the item that lies inside the utterance is stored exactly once, at its place in the frame's record, and
//     nothing is stored behind the utterance (the 16-lane row exchange in front of the whole-tile stores is modelled as
//     v_permlane16_swap defines it: odd rows of the first register <-> even rows of the second);
//   * the number of descriptor stores the wait behind the item counts (16 per whole row tile).
// No GPU, no HIP call.  Build and run under the host sanitizers:
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -Iinclude -Ifastdiff_amd/csrc tools/gemm16_index_check.cpp -o gemm16_index_check && ./gemm16_index_check
#include <cstdint>
#include <cstdio>
#include <vector>

#include "fd_kernels.h"
#include "fd_wpack.h"

using namespace fdk_fast;

static int failures = 0;
#define CHECK(cond, ...)                                                                                                                  \
    do {                                                                                                                                  \
        if (!(cond)) {                                                                                                                    \
            if (failures < 20) { std::printf("FAIL %s:%d: %s -- ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
            ++failures;                                                                                                                   \
        }                                                                                                                                 \
    } while (0)

// who holds what behind the exchange: register `part` of lane `lane` holds the value that register ct_src of lane lane_src computed
static void swapped_source(int part, int lane, int &ct_src, int &lane_src)
{
    const int row = lane >> 4;
    if (part == 0) {
        if (row & 1) { ct_src = 1; lane_src = lane - 16; }
        else { ct_src = 0; lane_src = lane; }
    } else {
        if (row & 1) { ct_src = 1; lane_src = lane; }
        else { ct_src = 0; lane_src = lane + 16; }
    }
}

static void check_T(int T)
{
    const int B = 1, P = gw_pairs(T), chunks = P / GW_PAIRS, XG = fd::KREC / 128;
    const int64_t image_bytes = (int64_t)fd::NBLK * B * P * GW_ROWB;
    const int64_t pack_f4 = (int64_t)(fd::KREC / 32) * 2 * 16 * 64;      // float4s of one block's gemm_w_pack
    const int64_t rec_floats = (int64_t)fd::NBLK * B * T * fd::KREC;
    const int WINB = GW_PAIRS * GW_ROWB;
    const int xgs[2] = {0, XG - 1};
    for (int blk = 0; blk < fd::NBLK; blk += fd::NBLK - 1)
        for (int chunk = 0; chunk < chunks; ++chunk)
            for (int xi = 0; xi < 2; ++xi)
                for (int wave = 0; wave < 4; ++wave) {
                    const int xg = xgs[xi], ptile = xg * 4 + wave, b = 0, Tb = T;
                    const int64_t window = (((int64_t)blk * B + b) * P + (int64_t)chunk * GW_PAIRS) * GW_ROWB;
                    CHECK(window + WINB <= image_bytes, "T %d chunk %d: the window DMA reads behind the image", T, chunk);
                    const int t_begin = chunk * 2 * GW_PAIRS;
                    const int64_t krow = (((int64_t)blk * B + b) * T + t_begin) * fd::KREC + (int64_t)ptile * 32;
                    std::vector<int> produced((size_t)2 * GW_PAIRS * 32, 0);      // [frame of the item][position of the 32-column tile]
                    int n_fast = 0;
                    bool counted = true;
                    for (int rt = 0; rt < 2; ++rt) {
                        const int t0 = t_begin + 32 * rt;
                        if (t0 >= Tb) continue;
                        const bool whole = t0 + 32 <= Tb;
                        // operands
                        for (int lane = 0; lane < 64; ++lane)
                            for (int j = 0; j < 4; ++j)
                                for (int ks = 0; ks < 2; ++ks)
                                    for (int q = 0; q < 2; ++q) {
                                        const int off = rt * 16 * GW_ROWB + j * 256 + gw16_a_off(lane, q, ks);
                                        CHECK(off >= 0 && off + 16 <= WINB, "T %d: A read at %d outside the window", T, off);
                                        CHECK(window + off + 16 <= image_bytes, "T %d: A read outside the image", T);
                                        const int pair = chunk * GW_PAIRS + 16 * rt + (lane & 15), grp = 4 * ks + (lane >> 4);     // K group of 8 channels
                                        const int64_t want = (int64_t)pair * GW_ROWB + j * 256 + (((8 * q + grp) ^ (pair & 15)) << 4);     // k_h_wino's slot
                                        CHECK((int64_t)chunk * WINB + off == want, "T %d lane %d: A read is not (pair %d, j %d, piece %d, group %d)", T, lane,
                                              pair, j, q, grp);
                                        for (int ct = 0; ct < 2; ++ct) {
                                            const int64_t idx = gw16_b_idx(ptile, q, j, ks, ct, lane);
                                            CHECK(idx >= 0 && idx < pack_f4, "T %d: B read %lld outside the pack", T, (long long)idx);
                                            const int64_t tile0 = ((int64_t)ptile * 2 + q) * 16 * 64;
                                            CHECK(idx >= tile0 && idx < tile0 + 16 * 64, "T %d: B read outside (tile %d, piece %d)", T, ptile, q);
                                            const fdp::Op16 o = fdp::op16((int)(idx - tile0) * 8);
                                            CHECK(o.row == 16 * ct + (lane & 15) && o.k == 64 * j + 32 * ks + 8 * (lane >> 4),
                                                  "T %d lane %d: B read is column %d, k %d", T, lane, o.row, o.k);
                                        }
                                    }
                        // stores
                        for (int odd = 0; odd < 2; ++odd)
                            for (int i = 0; i < 4; ++i)
                                for (int h = 0; h < 2; ++h)      // whole: part; else: ct
                                    for (int lane = 0; lane < 64; ++lane) {
                                        int ct = h, src = lane;
                                        int64_t off = 0;
                                        if (whole) {
                                            swapped_source(h, lane, ct, src);
                                            CHECK(src >= 0 && src < 64, "lane %d", lane);
                                            off = (int64_t)gw16_st_lane_off(lane) + gw16_st_row_off(rt, h, i, odd);
                                            CHECK(off >= 0 && off < (int64_t)2 * GW_PAIRS * fd::KREC, "T %d: store outside the descriptor's range", T);
                                        }
                                        const int f = 2 * (16 * rt + gw16_d_pair(src, i)) + odd, pos = gw16_d_pos(src, ct);     // what the value is
                                        if (!whole) {
                                            if (!(t_begin + f < Tb)) continue;
                                            off = (int64_t)f * fd::KREC + pos;
                                        }
                                        CHECK(off == (int64_t)f * fd::KREC + pos, "T %d rt %d lane %d reg %d.%d: stored at %lld, is (frame %d, position %d)", T, rt,
                                              lane, h, i, (long long)off, f, pos);
                                        CHECK(t_begin + f < Tb, "T %d: frame %d stored behind the utterance", T, t_begin + f);
                                        CHECK(krow + off >= 0 && krow + off < rec_floats, "T %d: store outside the records", T);
                                        CHECK(krow + off < (((int64_t)blk * B + b) * T + T) * fd::KREC, "T %d: store outside the utterance's records", T);
                                        if (f >= 0 && f < 2 * GW_PAIRS && pos >= 0 && pos < 32) ++produced[(size_t)f * 32 + pos];
                                    }
                        if (whole) ++n_fast;
                        else counted = false;
                    }
                    for (int f = 0; f < 2 * GW_PAIRS; ++f)
                        for (int pos = 0; pos < 32; ++pos)
                            CHECK(produced[(size_t)f * 32 + pos] == (t_begin + f < Tb ? 1 : 0), "T %d chunk %d: (frame %d, position %d) produced %d times", T,
                                  chunk, t_begin + f, pos, produced[(size_t)f * 32 + pos]);
                    // the wait behind the item: 16 descriptor stores per whole row tile, vmcnt(0) otherwise
                    const int frames_in = Tb - t_begin < 64 ? Tb - t_begin : 64;
                    CHECK(!counted || n_fast * 32 == frames_in, "T %d chunk %d: %d row tiles counted for %d frames", T, chunk, n_fast, frames_in);
                    CHECK(counted == (frames_in % 32 == 0), "T %d chunk %d", T, chunk);
                }
}

int main()
{
    const int Ts[] = {1, 31, 32, 33, 63, 64, 65, 864};
    for (int T : Ts) {
        const int before = failures;
        check_T(T);
        std::printf("T = %3d: %s\n", T, failures == before ? "ok" : "FAILED");
    }
    if (failures) std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
