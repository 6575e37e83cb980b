// nnls_host_check.cpp -- a host program with its own main() that exercises fastdiff_amd/csrc/fd_nnls.h, the host side of
// fd_mel_to_linear_nnls:
//   * refusal(): every border accepted, one step outside refused with the value in the text; first_nonfinite() finds NaN and both
//     infinities by their bits and nothing else;
//   * step_bound(): for a triangular bank like the front-end's, a dense Gaussian bank of mixed sign and a rank-one bank, L lies in
//     [lambda_max, 1.02 lambda_max] of the Gram matrix, lambda_max from a cyclic Jacobi eigenvalue iteration written here; the same
//     bank gives the same bits twice; a zero bank gives a positive L and a finite step;
//   * betas(): beta_0 = 0, the closed form of the first values, increasing, below 1, and (k - 1) / (k + 2)-like growth;
//   * table() / fill_table(): AT and AP hold every element of the bank where the kernel reads it and zeros elsewhere; every index the
//     kernel forms for its A operands (the waves' pair ranges with the one-chunk look-ahead, the bin tiles) stays inside the table,
//     the pair ranges tile [0, KPAIRS) in whole chunks and every bin belongs to exactly one (wave, tile, register, lane half);
//   * lds() / layout(): the slots are in order and disjoint, LDS fits in 160 KiB with the doubles of the record pass 8-byte aligned
//     inside the partial sums' slot, and a scratch buffer of exactly `total` bytes is written at the last byte of every slot.
// No GPU, no HIP call.  Build and run under the host sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Ifastdiff_amd/csrc \
//       tools/nnls_host_check.cpp -o nnls_host_check && ./nnls_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <set>
#include <vector>

#include "fd_nnls.h"

static long checks = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        ++checks;                                                                   \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

using namespace fdn;

static bool refused(int B, int T, int it, int variant, const char *needle)
{
    char msg[MSG];
    const char *why = refusal(B, T, it, variant, msg);
    return why && strstr(why, needle);
}

// a small deterministic generator (no <random>: the same numbers everywhere)
static uint64_t lcg_state = 0x243F6A8885A308D3ull;
static double uniform() { lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull; return (double)(lcg_state >> 11) / 9007199254740992.0; }
static double gauss() { const double u = uniform() + 1e-300, v = uniform(); return sqrt(-2.0 * log(u)) * cos(6.283185307179586 * v); }

// the largest eigenvalue of bank bank^T by cyclic Jacobi rotations
static double jacobi_lambda_max(const std::vector<float> &bank)
{
    const int n = MELS;
    std::vector<double> G((size_t)n * n);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            double s = 0.0;
            for (int k = 0; k < BINS; ++k) s += (double)bank[(size_t)i * BINS + k] * (double)bank[(size_t)j * BINS + k];
            G[(size_t)i * n + j] = s;
        }
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < n; ++p)
            for (int q = p + 1; q < n; ++q) off += G[(size_t)p * n + q] * G[(size_t)p * n + q];
        if (off < 1e-300) break;
        for (int p = 0; p < n; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = G[(size_t)p * n + q];
                if (apq == 0.0) continue;
                const double theta = (G[(size_t)q * n + q] - G[(size_t)p * n + p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < n; ++k) {
                    const double gkp = G[(size_t)k * n + p], gkq = G[(size_t)k * n + q];
                    G[(size_t)k * n + p] = c * gkp - s * gkq;
                    G[(size_t)k * n + q] = s * gkp + c * gkq;
                }
                for (int k = 0; k < n; ++k) {
                    const double gpk = G[(size_t)p * n + k], gqk = G[(size_t)q * n + k];
                    G[(size_t)p * n + k] = c * gpk - s * gqk;
                    G[(size_t)q * n + k] = s * gpk + c * gqk;
                }
            }
    }
    double m = G[0];
    for (int i = 1; i < n; ++i) m = G[(size_t)i * n + i] > m ? G[(size_t)i * n + i] : m;
    return m;
}

int main()
{
    char msg[MSG];
    CHECK(sizeof(fd_nnls) == 32 && MELS == 80 && BINS == 513 && TILE == 32 && WAVES == 4 && KPAIRS == 260 && YROWS == 520 && MPAD == 96 && BPAD == 544);
    CHECK(DEFAULT_ITERS == 128 && MAX_ITERS == 4096 && POWER_ITERS == 200 && MARGIN == 1.01);
    CHECK(!refusal(1, 1, 0, FD_GL_PWG, msg) && !refusal(MAX_B, MAX_T, MAX_ITERS, FD_GL_TACOTRON, msg));
    CHECK(refused(0, 5, 3, 0, "B = 0") && refused(MAX_B + 1, 5, 3, 0, "B = 4097") && refused(1, 0, 3, 0, "T = 0") && refused(1, MAX_T + 1, 3, 0, "T = 1048577"));
    CHECK(refused(1, 5, -1, 0, "n_iters = -1") && refused(1, 5, MAX_ITERS + 1, 0, "n_iters = 4097") && refused(1, 5, 3, 2, "variant 2") && refused(1, 5, 3, -1, "variant -1"));
    {
        float a[6] = {0.0f, -0.0f, 1e38f, -1e-45f, 3.0f, 5.0f};
        CHECK(first_nonfinite(a, 6) == -1);
        a[4] = std::numeric_limits<float>::quiet_NaN();
        CHECK(first_nonfinite(a, 6) == 4);
        a[2] = -std::numeric_limits<float>::infinity();
        CHECK(first_nonfinite(a, 6) == 2 && first_nonfinite(a, 2) == -1 && first_nonfinite(a, 0) == -1);
    }

    std::vector<float> tri((size_t)MELS * BINS, 0.0f), dense((size_t)MELS * BINS), one((size_t)MELS * BINS), zero((size_t)MELS * BINS, 0.0f);
    for (int m = 0; m < MELS; ++m) {                        // overlapping triangles of growing width, like the front-end's
        const double lo = 2.0 + 6.0 * m * (1.0 + m / 160.0) * 0.66, mid = lo + 3.0 + m / 8.0, hi = mid + 3.0 + m / 8.0;
        for (int k = 0; k < BINS; ++k) {
            const double w = fmin((k - lo) / (mid - lo), (hi - k) / (hi - mid));
            if (w > 0.0) tri[(size_t)m * BINS + k] = (float)(w * 2.0 / (hi - lo));
        }
    }
    for (auto &v : dense) v = (float)(gauss() / 16.0);
    for (int m = 0; m < MELS; ++m)
        for (int k = 0; k < BINS; ++k) one[(size_t)m * BINS + k] = (float)((1.0 + m % 3) * (0.5 + (k % 7) / 7.0));
    for (const std::vector<float> *bank : {&tri, &dense, &one}) {
        const double lam = jacobi_lambda_max(*bank), L = step_bound(bank->data());
        CHECK(lam > 0.0 && L >= lam && L <= 1.02 * lam);
        CHECK(L == step_bound(bank->data()));               // deterministic
        const float s = step(L);
        CHECK(s > 0.0f && finite_bits(s) && fabs((double)s * L - 1.0) < 1e-6);
    }
    CHECK(step_bound(zero.data()) > 0.0 && finite_bits(step(step_bound(zero.data()))));

    {
        std::vector<float> b(MAX_ITERS);
        betas(MAX_ITERS, b.data());
        const double t1 = (1.0 + sqrt(5.0)) / 2.0, t2 = (1.0 + sqrt(1.0 + 4.0 * t1 * t1)) / 2.0;
        CHECK(b[0] == 0.0f && b[1] == (float)((t1 - 1.0) / t2));
        for (int k = 1; k < MAX_ITERS; ++k) CHECK(b[k] >= b[k - 1] && b[k] < 1.0f);
        CHECK(b[127] > 0.97f && b[MAX_ITERS - 1] > 0.999f);
        std::vector<float> few(3);
        betas(3, few.data());                               // exactly 3: the sanitizer sees a write behind it
        CHECK(few[2] == b[2]);
    }

    {   // the table and every index the kernel forms into it
        const Table t = table();
        CHECK(t.at == 0 && t.ap == (size_t)YROWS * MPAD && t.beta == t.ap + (size_t)MELS * BPAD && t.total == t.beta + MAX_ITERS);
        std::vector<float> tab(t.total);                    // exactly
        fill_table(dense.data(), tab.data());
        for (int k = 0; k < YROWS; ++k)
            for (int m = 0; m < MPAD; ++m) CHECK(tab[t.at + (size_t)k * MPAD + m] == ((k < BINS && m < MELS) ? dense[(size_t)m * BINS + k] : 0.0f));
        for (int m = 0; m < MELS; ++m)
            for (int k = 0; k < BPAD; ++k) CHECK(tab[t.ap + (size_t)m * BPAD + k] == (k < BINS ? dense[(size_t)m * BINS + k] : 0.0f));
        CHECK(tab[t.beta] == 0.0f && tab[t.beta + 1] > 0.28f && tab[t.beta + 1] < 0.29f);
        CHECK(pair_begin(0) == 0 && pair_begin(WAVES) == KPAIRS);
        std::set<int> bins;
        for (int w = 0; w < WAVES; ++w) {
            const int kb = pair_begin(w), ke = pair_begin(w + 1);
            CHECK(kb < ke && kb % CHUNK == 0 && ke % CHUNK == 0);
            for (int hi = 0; hi < 2; ++hi)
                for (int col = 0; col < 32; ++col) {
                    for (int kk = kb; kk < ke; ++kk)        // A y: the look-ahead reads pairs below ke only
                        for (int mt = 0; mt < MTILES; ++mt) {
                            const size_t i = t.at + (size_t)hi * MPAD + col + (size_t)2 * kk * MPAD + 32 * mt;
                            CHECK(i < t.ap);
                            tab.data()[i] += 0.0f;
                        }
                    CHECK(hi * TILE + col + 2 * (ke - 1) * TILE < YROWS * TILE);      // ... and y's rows in LDS
                    for (int kk = 0; kk < MELS / 2; ++kk)   // A^T r
                        for (int i5 = 0; i5 < bin_tiles(w); ++i5) {
                            const size_t i = t.ap + (size_t)hi * BPAD + 32 * w + col + (size_t)2 * kk * BPAD + 128 * i5;
                            CHECK(i < t.beta);
                            tab.data()[i] += 0.0f;
                        }
                }
            CHECK(bin_tiles(w) == (w == 0 ? 5 : 4) && bin_tiles(w) <= MAX_BT);
            for (int i5 = 0; i5 < bin_tiles(w); ++i5)
                for (int hi = 0; hi < 2; ++hi)
                    for (int v = 0; v < 16; ++v) {
                        const int bin = 32 * (w + 4 * i5) + (v & 3) + 8 * (v >> 2) + 4 * hi;
                        CHECK(bin < BPAD && bins.insert(bin).second);
                        if (i5 < MAX_BT - 1) CHECK(bin < BINS);      // only tile 16 reaches past the last bin
                    }
        }
        CHECK((int)bins.size() == BPAD && *bins.begin() == 0);
        const int counts[WAVES] = {(pair_begin(1) - pair_begin(0)) * MTILES + 40 * 5, (pair_begin(2) - pair_begin(1)) * MTILES + 40 * 4,
                                   (pair_begin(3) - pair_begin(2)) * MTILES + 40 * 4, (pair_begin(4) - pair_begin(3)) * MTILES + 40 * 4};
        CHECK(counts[0] == 356 && counts[1] == 364 && counts[2] == 364 && counts[3] == 376);
    }

    {
        const Lds o = lds();
        CHECK(o.y == 0 && o.part == (size_t)YROWS * TILE && o.r == o.part + (size_t)WAVES * MELS * TILE && o.g == o.r + (size_t)MELS * TILE && o.total == o.g + (size_t)MELS * TILE);
        CHECK(sizeof(float) * o.total <= 160 * 1024 && (sizeof(float) * o.part) % 8 == 0 && sizeof(double) * MELS * TILE <= sizeof(float) * (o.r - o.part));
        for (int B : {1, 3, 8, 31})
            for (int T : {1, 5, 37, 865}) {
                const Layout l = layout(B, T);
                CHECK(l.lens == 0 && l.part % 256 == 0 && l.part >= sizeof(int64_t) * (size_t)B && l.total >= l.part + sizeof(double) * 4 * (size_t)B * T);
                CHECK(layout(1, 1).lens == l.lens);         // the lens slot does not depend on the shape
                std::vector<unsigned char> buf(l.total);
                buf.data()[sizeof(int64_t) * (size_t)B - 1] = 1;
                buf.data()[l.part + sizeof(double) * 4 * (size_t)B * T - 1] = 1;
            }
    }
    printf("nnls_host_check: %ld checks passed\n", checks);
    return 0;
}
