// gl_host_check.cpp -- a host program with its own main() that exercises fastdiff_amd/csrc/fd_gl.h, the host side of fd_griffin_lim:
//   * samples(): 256 (frames - 1), -1 below 2 frames; refusal(): every border accepted, one step outside refused with the value in the text;
//   * cover() and envelope(): for every padded position of items of 2 .. 41 frames the covering frames are exactly those whose window
//     holds the position, at most four; on the returned range [512, 512 + L) the envelope is at least 1.25 and equals 1.5 wherever
//     four frames overlap; the kernels' walk (m = 256 q + r, frames q - 3 .. q at n = 256 (q - t) + r) visits the same frames and
//     reads inside a frame buffer of exactly frames x 1024 floats;
//   * the indices of the inverse transform (fd_kernels_dft.h: idft_pass1, idft_pass2) stay inside the half spectrum, the tables and
//     the [17][32] step buffer, and every bin of the Hermitian extension is visited exactly once per output row;
//   * layout(): the slots are 256-byte aligned, in order, disjoint, and hold what the kernels index (a buffer of exactly `total` bytes
//     is written at the last byte of every slot);
//   * philox_counter(): distinct (frame, bin) pairs give distinct (call, word) pairs, the stream word is the stated one and differs
//     from the sampler's and the training draws', the id reaches the counter words the sampler puts it in.
// No GPU, no HIP call.  Build and run under the host sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Ifastdiff_amd/csrc \
//       tools/gl_host_check.cpp -o gl_host_check && ./gl_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>
#include <vector>

#include "fd_gl.h"

static long checks = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        ++checks;                                                                   \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

static bool refused(int B, int T, int it, int64_t pitch, const char *needle)
{
    char msg[fdgl::MSG];
    const char *why = fdgl::refusal(B, T, it, pitch, msg);
    return why && strstr(why, needle);
}

int main()
{
    using namespace fdgl;
    char msg[MSG];
    CHECK(sizeof(fd_gl) == 32 && N == 1024 && HOP == 256 && BINS == 513 && COVER == 4 && SEG == 1792 && CALLS_PER_FRAME == 129);
    CHECK(samples(1) == -1 && samples(0) == -1 && samples(-5) == -1 && samples(2) == 256 && samples(866) == 865 * 256);
    CHECK(samples(MAX_T) == (int64_t)256 * (MAX_T - 1) && DEFAULT_ITERS == 60);
    CHECK(!refusal(1, 2, 0, 256, msg) && !refusal(MAX_B, MAX_T, MAX_ITERS, samples(MAX_T), msg));
    CHECK(refused(0, 2, 0, 256, "B = 0") && refused(MAX_B + 1, 2, 0, 256, "B = 4097") && refused(1, 1, 0, 256, "T = 1") && refused(1, MAX_T + 1, 0, samples(MAX_T) + 256, "T = "));
    CHECK(refused(1, 2, -1, 256, "n_iters = -1") && refused(1, 2, MAX_ITERS + 1, 256, "n_iters = 10001") && refused(1, 5, 3, 1023, "wav_pitch = 1023"));

    for (int64_t frames = 2; frames <= 41; ++frames) {
        const int64_t L = samples(frames), span = N + HOP * (frames - 1);
        std::vector<float> F((size_t)frames * N, 1.0f);     // exactly: the sanitizer sees a read behind it
        for (int64_t m = 0; m < span; ++m) {
            int64_t lo, hi;
            cover(m, frames, &lo, &hi);
            CHECK(lo >= 0 && hi < frames && lo <= hi && hi - lo + 1 <= COVER);
            for (int64_t t = 0; t < frames; ++t) CHECK((m - HOP * t >= 0 && m - HOP * t < N) == (t >= lo && t <= hi));
            // the kernels' walk
            const int64_t q = m >> 8;
            const int r = (int)(m & 255);
            int64_t first = -1, last = -1;
            double sum = 0.0;
            for (int d = COVER - 1; d >= 0; --d) {
                const int64_t t = q - d;
                if (t < 0 || t >= frames) continue;
                if (first < 0) first = t;
                last = t;
                CHECK(256 * d + r < N);
                sum += F.data()[t * N + 256 * d + r];
            }
            CHECK(first == lo && last == hi && sum == (double)(hi - lo + 1));
            const double e = envelope(m, frames);
            if (m >= PAD && m < PAD + L) {
                CHECK(e >= 1.25 - 1e-12);
                if (hi - lo + 1 == COVER) CHECK(fabs(e - 1.5) < 1e-12);
            }
        }
        CHECK(fabs(envelope(PAD, frames) - 1.25) < 1e-12);
    }

    {   // the inverse transform's indices: k = k1 + 32 k2, rows k1 = 0 .. 16
        const int N1 = fdt::split_n1(N), N2 = fdt::split_n2(N), H = N1 / 2, G = THREADS / N2;
        CHECK(N1 == 32 && N2 == 32 && 2 * G == H);
        for (int k1 = 0; k1 <= H; ++k1) {
            std::set<int> seen;
            for (int k2 = 0; k2 < N2 / 2; ++k2) { const int k = k1 + N1 * k2; CHECK(k >= 0 && k <= N / 2); seen.insert(k); }
            for (int k2 = N2 / 2; k2 < N2; ++k2) {
                const int k = k1 + N1 * k2, idx = N - k1 - N1 * k2;
                CHECK(idx >= 0 && idx <= N / 2 && (k > N / 2 || (k == N / 2 && k1 == 0)) && idx == N - k);
                seen.insert(k);
            }
            CHECK((int)seen.size() == N2);
            for (int n2 = 0; n2 < N2; ++n2) CHECK(k1 * n2 < N && k1 * N2 + n2 < (H + 1) * N2);
        }
        std::set<int> rows;
        for (int tid = 0; tid < THREADS; ++tid) { rows.insert(tid / N2); rows.insert(tid / N2 + G); }
        rows.insert(H);
        CHECK((int)rows.size() == H + 1 && *rows.begin() == 0 && *rows.rbegin() == H);
        std::set<int> outs;
        for (int tid = 0; tid < THREADS; ++tid)
            for (int q = 0; q < 4; ++q) outs.insert(N2 * (tid / N2 + 8 * q) + tid % N2);
        CHECK((int)outs.size() == N && *outs.rbegin() == N - 1);
        std::vector<float> c(N), s(N);
        fdt::twiddles(N, c.data(), s.data());
        for (int j = 0; j < N1; ++j) CHECK(c[N2 * j] == (float)cos(2.0 * 3.14159265358979323846 * j / N1) && s[N2 * j] == (float)sin(2.0 * 3.14159265358979323846 * j / N1));
        const size_t lds = sizeof(float) * (3 * N + 2 * 32 + SEG + N + 2 * 32 * fdt::row(N) + 2 * (BINS + 3) + 2 * (H + 1) * N2);
        CHECK(lds <= 40 * 1024 && 4 * lds <= 160 * 1024);   // four workgroups of the iteration kernel per CU
    }

    for (int B : {1, 3, 8})
        for (int T : {2, 5, 37, 865}) {
            const Layout o = layout(B, T);
            const size_t bt = (size_t)B * T;
            const size_t starts[6] = {o.lens, o.ids, o.amp, o.frames[0], o.frames[1], o.part};
            const size_t sizes[6] = {8 * (size_t)B, 8 * (size_t)B, 4 * bt * AMP_PITCH, 4 * bt * N, 4 * bt * N, 8 * bt * 4};
            std::vector<unsigned char> buf(o.total);
            for (int i = 0; i < 6; ++i) {
                CHECK(starts[i] % 256 == 0 && (i == 0 ? starts[i] == 0 : starts[i] >= starts[i - 1] + sizes[i - 1]) && starts[i] + sizes[i] <= o.total);
                buf.data()[starts[i] + sizes[i] - 1] = 1;
            }
            CHECK(AMP_PITCH >= BINS && AMP_PITCH % 4 == 0);
        }
    CHECK(layout(8, 865).frames[1] - layout(8, 865).frames[0] == align256((size_t)8 * 865 * N * 4));

    {   // the counter layout
        std::set<std::pair<uint64_t, int>> seen;
        for (int64_t t = 0; t < 40; ++t)
            for (int k = 0; k < BINS; ++k) {
                CHECK(philox_word(k) == k % 4 && philox_pos(t, k) == (uint64_t)(129 * t + k / 4));
                seen.insert({philox_pos(t, k), philox_word(k)});
            }
        CHECK(seen.size() == (size_t)40 * BINS);
        uint32_t c[4], key[2];
        philox_counter(0x1122334455667788ull, 0xAABBCCDD00000003ull, 7, 513 - 1, c, key);
        CHECK(c[0] == 129 * 7 + 128 && c[1] == (0u ^ 0x00000003u) && c[2] == 0xFFFFFFF8u && c[3] == (0x5EEDu ^ 0xAABBCCDDu));
        CHECK(key[0] == 0x55667788u && key[1] == 0x11223344u);
        philox_counter(1, 0, ((int64_t)1 << 32) / 129 + 1, 0, c, key);
        CHECK(c[1] == 1u);                                  // the position's high word
        CHECK(FD_GL_PHILOX_STREAM != 0xFFFFFFFFu && FD_GL_PHILOX_STREAM < 0xFFFFFFF9u && FD_GL_PHILOX_STREAM > (uint32_t)MAX_ITERS);
    }
    printf("gl_host_check: %ld checks passed\n", checks);
    return 0;
}
