// spectral_host_check.cpp -- a host program with its own main() that exercises fastdiff_amd/csrc/fd_spectral.h, the host side of
// fd_spectral_measure, over the accepted range of configurations:
//   * refusal(): every accepted (nfft, hop, win) border is accepted, one step outside is refused with the value in the text;
//   * frames(), short_len(), win_offset(), n1_range(): every sample under the window lies in an n1 the first pass visits;
//   * tables(): built for EVERY accepted (nfft, win) into a buffer of exactly table_floats(nfft) floats -- the window is zero outside
//     [offset, offset + win) and within [0, 1] inside, cos^2 + sin^2 = 1 to float32 rounding;
//   * the table indices the kernel forms (W_N1^(n1 k1), W_nfft^(n2 k1), W_N2^(n2 k2)) stay inside the table, through fd_dft.h, which
//     describes the transform the kernel shares with the mel front-end and STOI -- so also over the ranges those two use;
//   * every table that goes through fdt::twiddles (fdx::tables for every accepted (nfft, win), fds::tables, the mel front-end's cos and
//     sin) equals, bit for bit, the formula each builder spelled out before they shared it, restated here;
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
#include "fd_stoi.h"

static long checks = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        ++checks;                                                                   \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

static const double PI = 3.14159265358979323846;

static bool same_bits(float a, float b) { return memcmp(&a, &b, sizeof(a)) == 0; }

// cos and sin [nfft] hold, bit for bit, what every table builder computed before fdt::twiddles: the formula restated
static bool parents_twiddles(int nfft, const float *c, const float *s)
{
    for (int m = 0; m < nfft; ++m)
        if (!same_bits(c[m], (float)cos(2.0 * PI * m / nfft)) || !same_bits(s[m], (float)sin(2.0 * PI * m / nfft))) return false;
    return true;
}

// every index that the shared transform (fd_kernels_dft.h) forms over the n1 in [n1_lo, n1_hi) and the k2 <= k2_max of a caller whose
// frame holds frame_floats floats: inside the frame, the cos / sin table and the padded first-pass result
static void transform_indices(int nfft, int n1_lo, int n1_hi, int k2_max, int frame_floats)
{
    const int N1 = fdt::split_n1(nfft), N2 = fdt::split_n2(nfft), ROW = fdt::row(nfft);
    CHECK(N1 * N2 == nfft && ROW >= N1 && fdt::lds_floats(nfft) == 3 * (size_t)nfft + 2 * (size_t)N2 * ROW);
    CHECK(0 <= n1_lo && n1_lo < n1_hi && n1_hi <= N1 && k2_max < N2);
    for (int n1 = n1_lo; n1 < n1_hi; ++n1) {
        for (int n2 = 0; n2 < N2; ++n2) CHECK(N2 * n1 + n2 < frame_floats);
        for (int k1 = 0; k1 < N1; ++k1) CHECK(((n1 * k1) & (N1 - 1)) * N2 < nfft);
    }
    for (int n2 = 0; n2 < N2; ++n2) {
        for (int k1 = 0; k1 < N1; ++k1) CHECK(n2 * k1 < nfft && n2 * ROW + k1 < N2 * ROW);
        for (int k2 = 0; k2 <= k2_max; ++k2) CHECK(((n2 * k2) & (N2 - 1)) * N1 < nfft);
    }
}

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
        const int N1 = fdt::split_n1(nfft), N2 = fdt::split_n2(nfft);
        CHECK(N1 * N2 == nfft && 256 % N2 == 0 && 256 % N1 == 0);
        CHECK(fdx::lds_bytes(nfft) <= fdx::LDS_WORKGROUP_MAX && 2 * fdx::lds_bytes(nfft) <= 160 * 1024);
        // the borders of the accepted range, and one step outside
        CHECK(!fdx::refusal(one(nfft, fdx::HOP_MIN, fdx::WIN_MIN), msg) && !fdx::refusal(one(nfft, nfft, nfft), msg));
        CHECK(refused(one(nfft, fdx::HOP_MIN - 1, 240), "hop[0] = 15") && refused(one(nfft, nfft + 1, 240), "hop[0] = "));
        CHECK(refused(one(nfft, 50, 1), "win[0] = 1") && refused(one(nfft, 50, nfft + 1), "win[0] = "));
        CHECK(refused(one(nfft + 256, 50, 240), "nfft[0] = ") && refused(one(nfft, 50, 240, 0.0), "floor = 0") && refused(one(nfft, 50, 240, -1.0), "floor = -1"));
        CHECK(refused(one(nfft, 50, 240, NAN), "floor = ") && refused(one(nfft, 50, 240, INFINITY), "floor = inf"));
        transform_indices(nfft, 0, N1, N2 / 2, nfft);       // the kernel's table and LDS indices
        for (int win = fdx::WIN_MIN; win <= nfft; ++win) {
            std::vector<float> tab(fdx::table_floats(nfft));      // exactly: the sanitizer sees a write behind it
            fdx::tables(nfft, win, tab.data());
            for (int i = 0; i < win; ++i) CHECK(same_bits(tab[(nfft - win) / 2 + i], (float)(0.5 - 0.5 * cos(2.0 * PI * i / win))));
            CHECK(parents_twiddles(nfft, tab.data() + nfft, tab.data() + 2 * nfft));
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
    // the other two callers of the shared transform: the mel front-end (all 32 n1, k2 <= 16) and STOI (256 samples: n1 < 8; k2 < 14)
    transform_indices(1024, 0, 32, 16, 1024);
    transform_indices(fds::NFFT, 0, fds::FRAME / fdt::split_n2(fds::NFFT), 13, fds::FRAME);
    {   // their tables: cos, sin (mel; its window is built next to the upload in fd_api_ext.cpp) and window [256], cos, sin (STOI)
        std::vector<float> mel(2 * 1024), st(fds::TAB_FLOATS);
        fdt::twiddles(1024, mel.data(), mel.data() + 1024);
        CHECK(parents_twiddles(1024, mel.data(), mel.data() + 1024));
        fds::tables(st.data());
        for (int i = 0; i < fds::FRAME; ++i) CHECK(same_bits(st[i], (float)(0.5 - 0.5 * cos(2.0 * PI * (i + 1) / (fds::FRAME + 1)))));
        CHECK(parents_twiddles(fds::NFFT, st.data() + fds::FRAME, st.data() + fds::FRAME + fds::NFFT));
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
