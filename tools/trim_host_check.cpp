// trim_host_check.cpp -- a host program with its own main() that exercises fastdiff_amd/csrc/fd_trim.h, the host side of
// fd_trim_silences, and walks the index arithmetic of its kernels in buffers of exactly the kernels' sizes:
//   * windows(): W and M around every border, the refusals of refusal() one step outside each accepted range;
//   * mask(): against the plain definition written out again (counts over explicit index ranges, any-over-a-range);
//   * the mask kernel's prefix tables: ps[M], pm[M], kp[M + 1] filled as k_trim_mask fills them (prefix counts, differences clamped at
//     the ends, the edges mode from the first and last smoothed window) give fdtr::mask's flags and the kept samples per window;
//   * the gather's walk: for every tile of TILE outputs, the window of its first output by bisection, then run by run with the
//     neighbour-or-bisect step: every output index is written exactly once, from a source index inside its own window and inside n.
// No GPU, no HIP call.  Build and run under the host sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Ifastdiff_amd/csrc \
//       tools/trim_host_check.cpp -o trim_host_check && ./trim_host_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fd_trim.h"

static long checks = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        ++checks;                                                                   \
        if (!(cond)) {                                                              \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                                \
        }                                                                           \
    } while (0)

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(rng_state >> 33);
}

static int64_t find(const std::vector<int64_t> &kp, int64_t lo, int64_t hi, int64_t j)      // tr_find
{
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (kp.at(mid) <= j) lo = mid; else hi = mid;
    }
    return lo;
}

static void walk(int64_t n, int64_t W, const std::vector<uint8_t> &speech, int A, int G, int mode, int64_t L, int64_t TILE)
{
    int64_t M = 0;
    CHECK(fdtr::windows(n, 8000, 10, nullptr, &M) && (int64_t)speech.size() == M);
    std::vector<uint8_t> want(M);
    fdtr::mask(speech.data(), M, A, G, mode, want.data());
    // k_trim_mask, passes 2-4
    std::vector<int> ps(M), pm(M);
    std::vector<int64_t> kp(M + 1);
    int carry = 0;
    for (int64_t w = 0; w < M; ++w) ps[w] = (carry += speech[w] ? 1 : 0);
    int64_t first = M, last = -1;
    carry = 0;
    for (int64_t w = 0; w < M; ++w) {
        const int64_t lo = w - (A - 1) / 2, hi = w + A / 2;
        const int c = ps.at(hi < M - 1 ? hi : M - 1) - (lo > 0 ? ps.at(lo - 1) : 0);
        const int s = 2 * c > A;
        if (s) { if (w < first) first = w; last = w; }
        pm[w] = (carry += s);
    }
    const int64_t e_lo = first - G / 2, e_hi = last + G / 2;
    int64_t kcarry = 0;
    for (int64_t w = 0; w < M; ++w) {
        int keep;
        if (mode == fdtr::MODE_EDGES) {
            keep = last >= 0 && w >= e_lo && w <= e_hi;
        } else {
            const int64_t lo = w - G / 2, hi = w + G / 2;
            keep = pm.at(hi < M - 1 ? hi : M - 1) - (lo > 0 ? pm.at(lo - 1) : 0) > 0;
        }
        const int64_t take = keep ? (w < M - 1 ? W : n - w * W) : 0;
        kp[w] = kcarry;
        kcarry += take;
        const int sp = ps[w] - (w > 0 ? ps[w - 1] : 0), sm = pm[w] - (w > 0 ? pm[w - 1] : 0);
        CHECK((uint8_t)(sp | (sm << 1) | (keep << 2)) == want[w]);
    }
    kp[M] = kcarry;
    const int64_t n_out = kcarry;
    CHECK(n_out <= n);
    // k_trim_gather
    std::vector<int64_t> src_of(L, -2);                    // -2: never written, -1: zero
    for (int64_t t0 = 0; t0 < L; t0 += TILE) {
        if (t0 >= n_out) {
            for (int64_t j = t0; j < t0 + TILE && j < L; ++j) { CHECK(src_of.at(j) == -2); src_of[j] = -1; }
            continue;
        }
        const int64_t t_end = t0 + TILE < n_out ? t0 + TILE : n_out;
        int64_t pos = t0, w = find(kp, 0, M, t0);
        while (pos < t_end) {
            const int64_t k0 = kp.at(w), k1 = kp.at(w + 1);
            CHECK(k0 <= pos && pos < k1 && (want.at(w) & 4));
            const int64_t end = k1 < t_end ? k1 : t_end;
            for (int64_t j = pos; j < end; ++j) {
                const int64_t s = w * W - k0 + j;
                CHECK(src_of.at(j) == -2 && s >= w * W && s < (w < M - 1 ? (w + 1) * W : n));
                src_of[j] = s;
            }
            pos = end;
            if (pos < t_end) w = kp.at(w + 2) > pos ? w + 1 : find(kp, w + 1, M, pos);
        }
        for (int64_t j = t_end; j < t0 + TILE && j < L; ++j) { CHECK(src_of.at(j) == -2); src_of[j] = -1; }
    }
    int64_t j = 0;                                         // the outputs are the kept windows' samples in order, then zeros
    for (int64_t w = 0; w < M; ++w)
        if (want[w] & 4)
            for (int64_t s = w * W; s < (w < M - 1 ? (w + 1) * W : n); ++s) CHECK(src_of.at(j++) == s);
    CHECK(j == n_out);
    for (; j < L; ++j) CHECK(src_of.at(j) == -1);
}

int main()
{
    // windows and refusals
    for (int rate : {8000, 16000, 22050, 192000})
        for (int ms : {10, 20, 30}) {
            const int64_t W0 = (int64_t)ms * rate / 1000;
            for (int64_t n : {(int64_t)0, (int64_t)1, W0 - 1, W0, W0 + 1, 2 * W0 - 1, 2 * W0, 13 * W0 + 5}) {
                int64_t W = 0, M = 0;
                CHECK(fdtr::windows(n, rate, ms, &W, &M) && W == W0 && M == (n / W0 > 1 ? n / W0 : 1));
            }
        }
    CHECK(!fdtr::windows(-1, 22050, 30, nullptr, nullptr) && !fdtr::windows(1, 7999, 30, nullptr, nullptr) && !fdtr::windows(1, 192001, 30, nullptr, nullptr));
    CHECK(!fdtr::windows(1, 22050, 15, nullptr, nullptr) && fdtr::windows(1, 22050, 30, nullptr, nullptr));
    char why[fdtr::MSG];
    CHECK(!fdtr::refusal(22050, 30, 40.0, -70.0, 8, 12, 0, 0, why) && !fdtr::refusal(8000, 10, 1e-3, 0.0, 1, 0, 1, 0, why));
    CHECK(!fdtr::refusal(192000, 20, 40.0, -70.0, 64, 254, 0, 0, why));
    CHECK(fdtr::refusal(7999, 30, 40.0, -70.0, 8, 12, 0, 0, why) && strstr(why, "7999"));
    CHECK(fdtr::refusal(22050, 25, 40.0, -70.0, 8, 12, 0, 0, why) && strstr(why, "25"));
    CHECK(fdtr::refusal(22050, 30, 0.0, -70.0, 8, 12, 0, 0, why) && fdtr::refusal(22050, 30, 40.0, NAN, 8, 12, 0, 0, why));
    CHECK(fdtr::refusal(22050, 30, 40.0, -70.0, 0, 12, 0, 0, why) && fdtr::refusal(22050, 30, 40.0, -70.0, 65, 12, 0, 0, why));
    CHECK(fdtr::refusal(22050, 30, 40.0, -70.0, 8, 11, 0, 0, why) && fdtr::refusal(22050, 30, 40.0, -70.0, 8, 256, 0, 0, why));
    CHECK(fdtr::refusal(22050, 30, 40.0, -70.0, 8, -2, 0, 0, why) && fdtr::refusal(22050, 30, 40.0, -70.0, 8, 12, 2, 0, why));
    CHECK(fdtr::refusal(22050, 30, 40.0, -70.0, 8, 12, 0, 1, why));
    // mask() against the definition, then the kernels' walk
    const int64_t W = 80;
    for (int64_t M : {(int64_t)1, (int64_t)2, (int64_t)7, (int64_t)8, (int64_t)13, (int64_t)255, (int64_t)256, (int64_t)257, (int64_t)517})
        for (int trial = 0; trial < 6; ++trial) {
            std::vector<uint8_t> s(M);
            const unsigned dens = (unsigned[]){1, 3, 6, 9, 10, 0}[trial];      // tenths of speech; 0: none at all
            int64_t w = 0;
            while (w < M) {                                // stretches of random length: long gaps and long bursts both occur
                const int64_t len = 1 + rnd() % 40;
                const bool on = rnd() % 10 < dens;
                for (int64_t k = 0; k < len && w < M; ++k) s[w++] = on;
            }
            for (int A : {1, 7, 8, 64})
                for (int G : {0, 2, 12, 254})
                    for (int mode : {fdtr::MODE_LONG, fdtr::MODE_EDGES}) {
                        std::vector<uint8_t> f(M);
                        fdtr::mask(s.data(), M, A, G, mode, f.data());
                        std::vector<uint8_t> sm(M), keep(M);
                        for (int64_t i = 0; i < M; ++i) {
                            int c = 0;
                            for (int64_t v = i - (A - 1) / 2; v <= i + A / 2; ++v) c += v >= 0 && v < M && s[v];
                            sm[i] = 2 * c > A;
                        }
                        int64_t a = -1, b = -1;
                        for (int64_t i = 0; i < M; ++i) {
                            for (int64_t v = i - G / 2; v <= i + G / 2; ++v) keep[i] |= v >= 0 && v < M && sm[v];
                            if (keep[i]) { if (a < 0) a = i; b = i; }
                        }
                        for (int64_t i = 0; i < M; ++i) {
                            const bool k = mode == fdtr::MODE_EDGES ? (a >= 0 && i >= a && i <= b) : keep[i];
                            CHECK(f[i] == (uint8_t)((s[i] ? 1 : 0) | (sm[i] ? 2 : 0) | (k ? 4 : 0)));
                        }
                        for (int64_t r : {(int64_t)0, (int64_t)1, W - 1}) {
                            const int64_t n = M * W + r;
                            walk(n, W, s, A, G, mode, n + (trial % 2 ? 0 : 777), 2048);
                        }
                    }
        }
    {   // shorter than a window
        std::vector<uint8_t> s(1, 1);
        walk(1, W, s, 1, 0, fdtr::MODE_LONG, 1, 2048);
        walk(W - 1, W, s, 1, 0, fdtr::MODE_EDGES, W + 5, 2048);
    }
    printf("trim_host_check: %ld checks passed\n", checks);
    return 0;
}
