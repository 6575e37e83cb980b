// fd_trim.h -- host side of the silence trimmer (include/fastdiff_hip_ext.h: "Cutting long silences"): the limits, the parameter check,
// the window grid of an utterance, and steps 4-5 (smoothing, dilation, the edges mode) stated on the host.  Plain C++ without the HIP
// runtime, so a stand-alone host program can include it.  tests/trim_ref.py is the float64 oracle.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "fd_loudness.h"

namespace fdtr {

constexpr int CHUNK = 256;                                     // FD_TRIM_CHUNK: windows per pass of the mask kernel's workgroup
constexpr int MAX_AVERAGE = 64, MAX_SILENCE = 254;
constexpr int MODE_LONG = 0, MODE_EDGES = 1;
constexpr int64_t MAX_SAMPLES = 2147483647;                    // out_valid and the record count in int32
constexpr double E_FLOOR = 1e-20;
constexpr int MSG = 200;

inline bool window_ms_ok(int ms) { return ms == 10 || ms == 20 || ms == 30; }

// W = window_ms rate / 1000 and M = max(1, n / W), integer divisions; false: a rate or window the tool refuses, or n < 0
inline bool windows(int64_t n, int rate, int window_ms, int64_t *W, int64_t *M)
{
    if (n < 0 || !fdl::rate_ok(rate) || !window_ms_ok(window_ms)) return false;
    const int64_t w = (int64_t)window_ms * rate / 1000;
    if (W) *W = w;
    if (M) *M = n / w > 1 ? n / w : 1;
    return true;
}

// why a parameter set is refused (true), else false
inline bool refusal(int rate, int window_ms, double top_db, double floor_db, int average_width, int max_silence, int mode, int reserved, char *why)
{
    if (!fdl::rate_ok(rate)) { snprintf(why, MSG, "sample rate %d outside %d .. %d", rate, fdl::RATE_MIN, fdl::RATE_MAX); return true; }
    if (!window_ms_ok(window_ms)) { snprintf(why, MSG, "window_ms = %d, 10, 20 or 30 are supported", window_ms); return true; }
    if (!isfinite(top_db) || top_db <= 0.0) { snprintf(why, MSG, "top_db must be finite and positive"); return true; }
    if (!isfinite(floor_db)) { snprintf(why, MSG, "floor_db must be finite"); return true; }
    if (average_width < 1 || average_width > MAX_AVERAGE) { snprintf(why, MSG, "average_width = %d outside 1 .. %d", average_width, MAX_AVERAGE); return true; }
    if (max_silence < 0 || max_silence > MAX_SILENCE || (max_silence & 1)) {
        snprintf(why, MSG, "max_silence = %d: an even count of 0 .. %d windows is expected", max_silence, MAX_SILENCE);
        return true;
    }
    if (mode != MODE_LONG && mode != MODE_EDGES) { snprintf(why, MSG, "mode = %d (FD_TRIM_LONG / FD_TRIM_EDGES)", mode); return true; }
    if (reserved != 0) { snprintf(why, MSG, "reserved = %d, must be 0", reserved); return true; }
    return false;
}

// Steps 4-5 on the host: speech[M] (0 / 1) -> flags[M], bit 0 speech, bit 1 smooth, bit 2 keep.
//   c_w = speech flags among w - (A - 1) / 2 .. w + A / 2 (outside 0 .. M - 1: 0);  smooth_w = 2 c_w > A
//   keep_w = any smooth_v with |v - w| <= G / 2;  MODE_EDGES: every window from the first kept one to the last
inline void mask(const uint8_t *speech, int64_t M, int A, int G, int mode, uint8_t *flags)
{
    std::vector<uint8_t> smooth((size_t)M, 0);
    for (int64_t w = 0; w < M; ++w) {
        int c = 0;
        for (int64_t v = w - (A - 1) / 2; v <= w + A / 2; ++v) c += (v >= 0 && v < M && speech[v]) ? 1 : 0;
        smooth[w] = 2 * c > A;
    }
    int64_t first = M, last = -1;
    for (int64_t w = 0; w < M; ++w) {
        bool keep = false;
        for (int64_t v = w - G / 2; v <= w + G / 2 && !keep; ++v) keep = v >= 0 && v < M && smooth[v];
        flags[w] = (uint8_t)((speech[w] ? 1 : 0) | (smooth[w] ? 2 : 0) | (keep ? 4 : 0));
        if (keep) { if (first == M) first = w; last = w; }
    }
    if (mode == MODE_EDGES)
        for (int64_t w = first; w <= last; ++w) flags[w] |= 4;
}

}  // namespace fdtr
