// spectral_host_check.cpp -- a host program with its own main() that exercises fastdiff_amd/csrc/fd_spectral.h, the host side of
// fd_spectral_measure, over the accepted range of configurations:
//   * refusal(): every accepted (nfft, hop, win) border is accepted, one step outside is refused with the value in the text;
//   * frames(), short_len(), win_offset(), n1_range(): every sample under the window lies in an n1 the first pass visits;
//   * tables(): built for EVERY accepted (nfft, win) into a buffer of exactly table_floats(nfft) floats -- the window is zero outside
//     [offset, offset + win) and within [0, 1] inside, cos^2 + sin^2 = 1 to float32 rounding;
//   * the table indices the kernel forms (W_N1^(n1 k1), W_nfft^(n2 k1), W_N2^(n2 k2)) stay inside the table;
//   * the reflection rule of k_spectral_frames, walked for every frame and every sample under the window over signals of n samples
//     (n from short_len + 1 upwards) held in a buffer of exactly n floats: nothing at or behind n is read;
//   * lds_bytes(): within LDS_WORKGROUP_MAX, two of the largest within a CU's 160 KiB.
// No GPU, no HIP call.  Build and run under the host sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Ifastdiff_amd/csrc \
//       tools/spectral_host_check.cpp -o spectral_host_check && ./spectral_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fd_spectral.h"

static long checks = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        ++checks;                                                                   \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

static fd_spectral_config one(int nfft, int hop, int win, double floor_ = 1e-7)
{
    fd_spectral_config c;
    fdx::defaults(&c);
    c.n_res = 1; c.nfft[0] = nfft; c.hop[0] = hop; c.win[0] = win; c.floor = floor_;
    return c;
}

static bool refused(const fd_spectral_config &c, const char *needle)
{
    char msg[fdx::MSG];
    const char *why = fdx::refusal(c, msg);
    return why && strstr(why, needle);
}

int main()
{
    char msg[fdx::MSG];
    fd_spectral_config d;
    fdx::defaults(&d);
    CHECK(!fdx::refusal(d, msg) && d.n_res == 3 && fdx::short_len(d) == 1024 && d.floor == 1e-7);
    CHECK(sizeof(fd_spectral) == 144 && sizeof(fd_spectral) % 8 == 0 && sizeof(fd_spectral_config) == 64);
    const int nffts[3] = {512, 1024, 2048};
    for (int nfft : nffts) {
        const int N1 = fdx::split_n1(nfft), N2 = fdx::split_n2(nfft);
        CHECK(N1 * N2 == nfft && 256 % N2 == 0 && 256 % N1 == 0);
        CHECK(fdx::lds_bytes(nfft) <= fdx::LDS_WORKGROUP_MAX && 2 * fdx::lds_bytes(nfft) <= 160 * 1024);
        // the borders of the accepted range, and one step outside
        CHECK(!fdx::refusal(one(nfft, fdx::HOP_MIN, fdx::WIN_MIN), msg) && !fdx::refusal(one(nfft, nfft, nfft), msg));
        CHECK(refused(one(nfft, fdx::HOP_MIN - 1, 240), "hop[0] = 15") && refused(one(nfft, nfft + 1, 240), "hop[0] = "));
        CHECK(refused(one(nfft, 50, 1), "win[0] = 1") && refused(one(nfft, 50, nfft + 1), "win[0] = "));
        CHECK(refused(one(nfft + 256, 50, 240), "nfft[0] = ") && refused(one(nfft, 50, 240, 0.0), "floor = 0") && refused(one(nfft, 50, 240, -1.0), "floor = -1"));
        CHECK(refused(one(nfft, 50, 240, NAN), "floor = ") && refused(one(nfft, 50, 240, INFINITY), "floor = inf"));
        // the kernel's table indices
        for (int n1 = 0; n1 < N1; ++n1)
            for (int k1 = 0; k1 < N1; ++k1) CHECK(((n1 * k1) & (N1 - 1)) * N2 < nfft);
        for (int n2 = 0; n2 < N2; ++n2) {
            for (int k1 = 0; k1 < N1; ++k1) CHECK(n2 * k1 < nfft);
            for (int k2 = 0; k2 <= N2 / 2; ++k2) CHECK(((n2 * k2) & (N2 - 1)) * N1 < nfft);
        }
        for (int win = fdx::WIN_MIN; win <= nfft; ++win) {
            std::vector<float> tab(fdx::table_floats(nfft));      // exactly: the sanitizer sees a write behind it
            fdx::tables(nfft, win, tab.data());
            const int off = fdx::win_offset(nfft, win);
            int lo, hi;
            fdx::n1_range(nfft, win, &lo, &hi);
            CHECK(off >= 0 && off + win <= nfft && 0 <= lo && lo < hi && hi <= N1);
            for (int i = 0; i < nfft; ++i) {
                const bool under = i >= off && i < off + win;
                CHECK(under ? (tab[i] >= 0.0f && tab[i] <= 1.0f) : tab[i] == 0.0f);
                if (under) CHECK(i / N2 >= lo && i / N2 < hi);
                const double c = tab[nfft + i], s = tab[2 * nfft + i];
                CHECK(fabs(c * c + s * s - 1.0) < 3e-7);
            }
            CHECK(tab[off] == 0.0f && tab[nfft] == 1.0f && tab[2 * nfft] == 0.0f && tab[nfft + nfft / 2] == -1.0f);
        }
        // the reflection: every read lands inside the signal's own n samples
        const int hops[4] = {fdx::HOP_MIN, 50, nfft / 2 + 1, nfft};
        for (int hop : hops) {
            const int wins[3] = {fdx::WIN_MIN, nfft / 2 - 1, nfft};
            for (int win : wins) {
                const fd_spectral_config c = one(nfft, hop, win);
                CHECK(!fdx::refusal(c, msg));
                const int off = fdx::win_offset(nfft, win);
                const int64_t lens[5] = {fdx::short_len(c) + 1, fdx::short_len(c) + 2, nfft - 1, nfft + 1, 3 * (int64_t)nfft + 7};
                for (int64_t n : lens) {
                    std::vector<float> s((size_t)n, 1.0f);
                    const int64_t F = fdx::frames(n, hop);
                    CHECK(F == 1 + n / hop && (F - 1) * hop <= n);
                    double sum = 0.0;
                    for (int64_t f = 0; f < F; ++f)
                        for (int i = off; i < off + win; ++i) {
                            int64_t p = f * hop - nfft / 2 + i;
                            p = p < 0 ? -p : (p >= n ? 2 * (n - 1) - p : p);
                            CHECK(p >= 0 && p < n);
                            sum += s.data()[p];
                        }
                    CHECK(sum == (double)F * win);
                }
            }
        }
    }
    // the other refusals
    d.n_res = 0; CHECK(refused(d, "n_res = 0"));
    d.n_res = 5; CHECK(refused(d, "n_res = 5"));
    d.n_res = 3; d.reserved = 7; CHECK(refused(d, "reserved = 7"));
    for (int hop : {16, 50, 2048})
        for (int64_t k : {1, 2, 1000}) {
            CHECK(fdx::frames(hop * k - 1, hop) == k && fdx::frames(hop * k, hop) == k + 1 && fdx::frames(hop * k + 1, hop) == k + 1);
        }
    CHECK(fdx::frames(0, 50) == 1 && fdx::frames(fdx::MAX_SAMPLES, fdx::HOP_MIN) == (((int64_t)1 << 26) + 1));
    printf("spectral_host_check: %ld checks passed\n", checks);
    return 0;
}
