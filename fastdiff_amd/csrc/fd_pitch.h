// fd_pitch.h -- host side of the F0 tracker and the pitch scores (include/fastdiff_hip_ext.h: "F0 tracking"): the constants that decide
// which workgroup or wavefront handles which frame or lag, the derived lags with the refusals, and the frame count.
// Plain C++ without the HIP runtime, so a stand-alone host program can include it.  tests/pitch_ref.py is the float64 oracle.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/fastdiff_hip_ext.h"

namespace fdp {

constexpr int MAX_LAGS = 1024;                                // FD_PITCH_MAX_LAGS: the largest L = tau_max + 2
constexpr int FRAME_TILE = 4;                                 // FD_PITCH_FRAME_TILE: consecutive frames per workgroup of the tracker
constexpr int LAG_CHUNK = 64;                                 // FD_PITCH_LAG_CHUNK: lags per wavefront pass (a lane per lag)
constexpr int WIN_MIN = 64, WIN_MAX = 2048;
constexpr int STAGE_FLOATS = 6144;                            // FD_PITCH_STAGE_FLOATS: LDS floats for the samples of a tile (span <= 2048 + 1022 + 1 fits alone)
constexpr int64_t MAX_FRAMES = (int64_t)1 << 30;

struct Lags { int tau_min, tau_max, L, span; };

inline void defaults(fd_pitch_config *c)
{
    c->rate = 22050; c->hop = 256; c->win = 1024; c->reserved = 0;
    c->f0_min = 80.0; c->f0_max = 750.0; c->threshold = 0.15;
}

// the derived values; null = fine, else what is wrong with the configuration
inline const char *lags(const fd_pitch_config &c, Lags &o)
{
    o = Lags{0, 0, 0, 0};
    if (c.reserved != 0) return "reserved is not 0";
    if (c.rate < 1) return "rate < 1";
    if (!(c.f0_min > 0.0) || !(c.f0_max > 0.0)) return "f0_min and f0_max must be positive";
    if (!(c.threshold > 0.0 && c.threshold < 1.0)) return "threshold outside (0, 1)";
    if (c.hop < 1) return "hop < 1";
    if (c.win < WIN_MIN || c.win > WIN_MAX) return "win outside 64 .. 2048";
    const double lo = floor((double)c.rate / c.f0_max), hi = ceil((double)c.rate / c.f0_min);
    if (lo < 2.0) return "tau_min = floor(rate / f0_max) < 2";
    if (hi <= lo) return "tau_max = ceil(rate / f0_min) <= tau_min";
    if (hi + 2.0 > (double)MAX_LAGS) return "L = tau_max + 2 > FD_PITCH_MAX_LAGS";
    o.tau_min = (int)lo; o.tau_max = (int)hi; o.L = o.tau_max + 2; o.span = c.win + o.tau_max + 1;
    return nullptr;
}

inline int64_t frames(int64_t n, int hop) { return n / hop; }

// frames of a tile whose samples are staged together: the most g <= FRAME_TILE with span + (g - 1) hop <= STAGE_FLOATS
inline int stage_group(int span, int hop)
{
    const int64_t g = 1 + (STAGE_FLOATS - span) / (int64_t)hop;
    return (int)(g < FRAME_TILE ? g : FRAME_TILE);
}

// the dynamic LDS of the tracker in floats: [samples of a stage group | 4 wavefronts x L doubles of d'] then FRAME_TILE x L sums
inline int stage_floats(int span, int hop, int L)
{
    const int s = span + (stage_group(span, hop) - 1) * hop;
    return s > 8 * L ? s : 8 * L;
}
inline size_t lds_bytes(int span, int hop, int L) { return sizeof(float) * ((size_t)stage_floats(span, hop, L) + (size_t)FRAME_TILE * L); }

}  // namespace fdp
