// mcd_host_check.cpp -- a host program with its own main() that exercises fastdiff_amd/csrc/fd_mcd.h, the host side of fd_cepstra,
// fd_dtw and fd_mcd_measure:
//   * refusal(), coef_refusal(), wave_refusal(), dtw_refusal(), align_refusal(): every accepted border is accepted, one step outside
//     is refused with the value in the text;
//   * frames(): 1 + n / 256 around the hop;
//   * dct_table(): built into a buffer of exactly MAX_COEF x MELS floats; its rows, with row 0 from dct_entry, are orthonormal to
//     float32 rounding, and dct_entry's full 80 x 80 matrix is orthonormal to 1e-14;
//   * the skewed sweep of k_dtw, walked for Ta and Tb around ROWS, COLS and RING in buffers of exactly the kernel's sizes: in every step
//     of every row block the ring slot a thread reads holds the column it is at (b's ring and the ring of the row above), no tile load
//     overwrites a column that is still needed, the bottom row a block reads is the one the block before wrote (exactly Tb entries per
//     buffer, each written once), and the direction codes fill exactly code_bytes(Ta, Tb) bytes; the values that travel -- a thread's own last cell, the
//     cell above from its neighbour as of the step before, the diagonal one as the cell above of the step before -- give, on random
//     integer costs, the accumulated cost, path length and diagonal steps of the plain double loop with the header's tie rule, and the
//     walk back over the codes gives the alignment of that loop's back-tracked path;
//   * dtw_lds_bytes(): within LDS_WORKGROUP_MAX for both compiled widths.
// No GPU, no HIP call.  Build and run under the host sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Ifastdiff_amd/csrc \
//       tools/mcd_host_check.cpp -o mcd_host_check && ./mcd_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fd_mcd.h"

static long checks = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        ++checks;                                                                   \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

using namespace fdm;

static void refusals()
{
    char msg[MSG];
    fd_mcd_config c;
    defaults(&c);
    CHECK(c.n_coef == 13 && c.reserved == 0 && !refusal(c, msg));
    for (int n = 1; n <= MAX_COEF; ++n) { c.n_coef = n; CHECK(!refusal(c, msg)); }
    c.n_coef = 0;
    CHECK(refusal(c, msg) && strstr(msg, "n_coef = 0"));
    c.n_coef = MAX_COEF + 1;
    CHECK(refusal(c, msg) && strstr(msg, "n_coef = 41"));
    c.n_coef = 13; c.reserved = 3;
    CHECK(refusal(c, msg) && strstr(msg, "reserved = 3"));
    CHECK(!wave_refusal(1, 1, "L", msg) && !wave_refusal(MAX_B, MAX_FRAMES * HOP - 1, "L", msg));
    CHECK(wave_refusal(0, 1, "L", msg) && strstr(msg, "B = 0"));
    CHECK(wave_refusal(MAX_B + 1, 1, "L", msg) && strstr(msg, "B = 4097"));
    CHECK(wave_refusal(1, 0, "Lc", msg) && strstr(msg, "Lc = 0"));
    CHECK(wave_refusal(1, MAX_FRAMES * HOP, "L", msg) && strstr(msg, "L = 1073741824"));
    CHECK(!dtw_refusal(1, 1, 1, 1, 1, false, 0, msg) && !dtw_refusal(MAX_B, MAX_COEF, MAX_LD, MAX_FRAMES, MAX_FRAMES, true, MAX_FRAMES, msg));
    CHECK(dtw_refusal(1, 0, 1, 1, 1, false, 0, msg) && strstr(msg, "D = 0"));
    CHECK(dtw_refusal(1, MAX_COEF + 1, 64, 1, 1, false, 0, msg) && strstr(msg, "D = 41"));
    CHECK(dtw_refusal(1, 13, 12, 1, 1, false, 0, msg) && strstr(msg, "ld = 12"));
    CHECK(dtw_refusal(1, 13, MAX_LD + 1, 1, 1, false, 0, msg) && strstr(msg, "ld = 2097153"));
    CHECK(dtw_refusal(1, 13, 13, 0, 1, false, 0, msg) && strstr(msg, "pitch_a = 0"));
    CHECK(dtw_refusal(1, 13, 13, 1, MAX_FRAMES + 1, false, 0, msg) && strstr(msg, "pitch_b = 4194305"));
    CHECK(dtw_refusal(1, 13, 13, 9, 1, true, 8, msg) && strstr(msg, "align_pitch = 8"));
    CHECK(!align_refusal(0, 8192, 8192, msg) && !align_refusal(0, MAX_ALIGN_CELLS, 1, msg));
    CHECK(align_refusal(5, 8193, 8192, msg) && strstr(msg, "pair 5") && strstr(msg, "8193 x 8192 = 67117056"));
    for (int64_t k = 0; k < 5; ++k)
        for (int64_t n : {HOP * k - 1, HOP * k, HOP * k + 1})
            if (n >= 0) CHECK(frames(n) == 1 + n / HOP);
    CHECK(frames(0) == 1 && frames(255) == 1 && frames(256) == 2 && frames(513) == 3);
    CHECK(padded_d(1) == 16 && padded_d(16) == 16 && padded_d(17) == MAX_COEF && padded_d(MAX_COEF) == MAX_COEF);
    CHECK(dtw_lds_bytes(16) <= LDS_WORKGROUP_MAX && dtw_lds_bytes(MAX_COEF) <= LDS_WORKGROUP_MAX);
}

static void dct()
{
    std::vector<float> tab((size_t)MAX_COEF * MELS);       // exactly what dct_table fills
    dct_table(tab.data());
    for (int d = 1; d <= MAX_COEF; ++d)
        for (int j = 0; j < MELS; ++j) CHECK(tab[(d - 1) * MELS + j] == (float)dct_entry(d, j));
    for (int d = 0; d < MELS; ++d)
        for (int e = d; e < MELS; ++e) {
            double s = 0.0;
            for (int j = 0; j < MELS; ++j) s += dct_entry(d, j) * dct_entry(e, j);
            CHECK(fabs(s - (d == e ? 1.0 : 0.0)) <= 1e-14);
        }
    for (int d = 1; d <= MAX_COEF; ++d)
        for (int e = d; e <= MAX_COEF; ++e) {
            double s = 0.0;
            for (int j = 0; j < MELS; ++j) s += (double)tab[(d - 1) * MELS + j] * tab[(e - 1) * MELS + j];
            CHECK(fabs(s - (d == e ? 1.0 : 0.0)) <= 80 * 6e-8);
        }
}

struct Cell { long long D; int L, N; };

static unsigned rnd_state = 12345u;
static int rnd(int m) { rnd_state = rnd_state * 1664525u + 1013904223u; return (int)((rnd_state >> 8) % (unsigned)m); }

// the sweep as k_dtw schedules it, on integer costs, against the plain double loop
static void sweep(int64_t Ta, int64_t Tb)
{
    std::vector<int> cost((size_t)(Ta * Tb));
    for (auto &c : cost) c = rnd(4);                       // few values: many ties
    // the plain loop with the header's tie rule
    std::vector<Cell> ref((size_t)(Ta * Tb));
    std::vector<unsigned char> rdir((size_t)(Ta * Tb), 0);
    for (int64_t i = 0; i < Ta; ++i)
        for (int64_t j = 0; j < Tb; ++j) {
            Cell best{0, 0, 0};
            unsigned dir = 0;
            const bool hu = i > 0, hl = j > 0, hd = hu && hl;
            if (hd) { const Cell &p = ref[(i - 1) * Tb + j - 1]; best = {p.D, p.L, p.N + 1}; }
            if (hu && (!hd || ref[(i - 1) * Tb + j].D < best.D)) { best = ref[(i - 1) * Tb + j]; dir = 1; }
            if (hl && (!hu || ref[i * Tb + j - 1].D < best.D)) { best = ref[i * Tb + j - 1]; dir = 2; }
            ref[i * Tb + j] = {cost[i * Tb + j] + best.D, best.L + 1, best.N};
            rdir[i * Tb + j] = (unsigned char)dir;
        }
    // the kernel's buffers, exactly sized
    std::vector<int64_t> ring_col(RING, -1), up_col(RING, -1);      // which column a slot of b's ring / of the ring of the row above holds
    std::vector<Cell> up_ring(RING);
    std::vector<Cell> bot[2] = {std::vector<Cell>((size_t)Tb), std::vector<Cell>((size_t)Tb)};
    std::vector<char> bot_set[2] = {std::vector<char>((size_t)Tb, 0), std::vector<char>((size_t)Tb, 0)};
    std::vector<unsigned char> codes((size_t)code_bytes(Ta, Tb), 0xEE);
    std::vector<char> code_set((size_t)code_bytes(Ta, Tb), 0);
    const int64_t cp = code_pitch(Tb);
    Cell edge[2][WAVES];
    Cell final{-1, 0, 0};
    auto load = [&](int64_t lo, int64_t hi, int64_t k, int64_t s, int nr) {
        CHECK(hi - lo >= 1 && hi - lo <= COLS && hi <= Tb);
        for (int64_t j = lo; j < hi; ++j) {
            const int sl = slot(j);
            // the column the slot held is needed by no thread in this step or a later one: the oldest needed now is s - (nr - 1)
            CHECK(ring_col[sl] < 0 || s < 0 || ring_col[sl] < s - (nr - 1) || ring_col[sl] >= Tb);
            ring_col[sl] = j;
            if (k > 0) { CHECK(bot_set[(k - 1) & 1][j]); up_ring[sl] = bot[(k - 1) & 1][j]; up_col[sl] = j; }
        }
    };
    for (int64_t k = 0; k < blocks(Ta); ++k) {
        const int nr = block_rows(Ta, k);

        const int64_t i0 = k * ROWS, S = block_steps(Ta, Tb, k);
        CHECK(nr >= 1 && nr <= ROWS && (k + 1 == blocks(Ta) || nr == ROWS));
        std::fill(ring_col.begin(), ring_col.end(), -1);
        std::fill(bot_set[k & 1].begin(), bot_set[k & 1].end(), 0);
        load(0, Tb < COLS ? Tb : COLS, k, -1, nr);
        std::vector<Cell> cur(ROWS, Cell{0, 0, 0}), dg(ROWS, Cell{0, 0, 0});
        std::vector<unsigned> pk(ROWS, 0);
        for (int64_t s = 0; s < S; ++s) {
            std::vector<Cell> before = cur;                // every thread's value of the step before
            for (int r = 0; r < ROWS; ++r) {
                const int64_t j = s - r, i = i0 + r;
                const int lane = r % WAVE, wave = r / WAVE;
                Cell u = before[r > 0 ? r - 1 : 0];
                if (lane == 0) {
                    if (wave > 0) u = edge[(s + 1) & 1][wave - 1];
                    else if (k > 0 && j < Tb) { CHECK(up_col[slot(j)] == j); u = up_ring[slot(j)]; }
                }
                if (lane == 0 && wave > 0 && s > 0) CHECK(u.D == before[r - 1].D && u.L == before[r - 1].L && u.N == before[r - 1].N);
                if (r < nr && j >= 0 && j < Tb) {
                    CHECK(ring_col[slot(j)] == j);
                    const bool hu = i > 0, hl = j > 0, hd = hu && hl;
                    Cell best{0, 0, 0};
                    unsigned dir = 0;
                    if (hd) best = {dg[r].D, dg[r].L, dg[r].N + 1};
                    if (hu && (!hd || u.D < best.D)) { best = u; dir = 1; }
                    if (hl && (!hu || before[r].D < best.D)) { best = before[r]; dir = 2; }
                    cur[r] = {cost[i * Tb + j] + best.D, best.L + 1, best.N};
                    const Cell &w = ref[i * Tb + j];
                    CHECK(cur[r].D == w.D && cur[r].L == w.L && cur[r].N == w.N && dir == rdir[i * Tb + j]);
                    pk[r] |= dir << (2 * (int)(j & 3));
                    if ((j & 3) == 3 || j == Tb - 1) {
                        CHECK(!code_set[i * cp + (j >> 2)]);
                        codes[i * cp + (j >> 2)] = (unsigned char)pk[r];
                        code_set[i * cp + (j >> 2)] = 1;
                        pk[r] = 0;
                    }
                    if (k + 1 < blocks(Ta) && r == nr - 1) { CHECK(!bot_set[k & 1][j]); bot[k & 1][j] = cur[r]; bot_set[k & 1][j] = 1; }
                    if (i == Ta - 1 && j == Tb - 1) final = cur[r];
                }
                dg[r] = u;
            }
            for (int w = 0; w < WAVES; ++w) edge[s & 1][w] = cur[w * WAVE + WAVE - 1];
            int64_t lo, hi;
            if (tile_at(s, Tb, &lo, &hi)) load(lo, hi, k, s, nr);
        }
    }
    const Cell &w = ref[Ta * Tb - 1];
    CHECK(final.D == w.D && final.L == w.L && final.N == w.N && w.L == Ta + Tb - 1 - w.N);
    for (char c : code_set) CHECK(c);
    // the walk back
    std::vector<int> al((size_t)Ta, -1), want((size_t)Ta, -1);
    int64_t i = Ta - 1, j = Tb - 1, cells = 0;
    for (;;) {
        al[i] = (int)j;
        ++cells;
        if (i == 0 && j == 0) break;
        unsigned c = (codes[i * cp + (j >> 2)] >> (2 * (int)(j & 3))) & 3u;
        if (i == 0) c = 2; else if (j == 0) c = 1;
        CHECK(c == rdir[i * Tb + j]);
        if (c == 0) { --i; --j; } else if (c == 1) --i; else --j;
    }
    CHECK(cells == w.L);
    for (int64_t r = 0; r < Ta; ++r) CHECK(al[r] >= 0 && al[r] < Tb && (r == 0 || al[r] >= al[r - 1]));
    CHECK(al[0] == 0);
}

int main()
{
    refusals();
    dct();
    const int64_t ta[] = {1, 2, ROWS - 1, ROWS, ROWS + 1, 2 * ROWS, 2 * ROWS + 1};
    const int64_t tb[] = {1, 2, 3, 4, 5, COLS - 1, COLS, COLS + 1, 2 * COLS, ROWS, RING - 1, RING, RING + 1, 2 * RING + 3};
    for (int64_t a : ta)
        for (int64_t b : tb) sweep(a, b);
    printf("mcd_host_check: %ld checks passed\n", checks);
    return 0;
}
