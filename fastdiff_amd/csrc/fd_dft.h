// fd_dft.h -- host side of the one split DFT that the mel front-end, STOI and the STFT distances share (fd_kernels_dft.h is the device
// side and states the algorithm): the split, the row pad, the LDS it takes and the cos / sin table.  Plain C++ without the HIP runtime,
// so a stand-alone host program can include it (tools/spectral_host_check.cpp).
#pragma once
#include <math.h>
#include <stddef.h>

namespace fdt {

constexpr int THREADS = 256;                                  // the workgroup the device side is written for
// the split nfft = N1 x N2 (n = N2 n1 + n2, k = k1 + N1 k2); 0 for an nfft the transform does not take
constexpr int split_n1(int nfft) { return nfft == 512 ? 16 : (nfft == 1024 || nfft == 2048 ? 32 : 0); }
constexpr int split_n2(int nfft) { return split_n1(nfft) ? nfft / split_n1(nfft) : 0; }
// floats per row of the first pass' result [N2][row]: N1 padded by one against bank conflicts
constexpr int row(int nfft) { return split_n1(nfft) + 1; }
// LDS floats of the transform: cos, sin and the frame [nfft] each (a caller whose frame is shorter keeps less), re and im [N2][row]
constexpr size_t lds_floats(int nfft) { return 3 * (size_t)nfft + 2 * (size_t)split_n2(nfft) * row(nfft); }

// cos and sin of 2 pi m / nfft, m < nfft, rounded once from double
inline void twiddles(int nfft, float *cos_out, float *sin_out)
{
    const double pi = 3.14159265358979323846;
    for (int m = 0; m < nfft; ++m) {
        cos_out[m] = (float)cos(2.0 * pi * m / nfft);
        sin_out[m] = (float)sin(2.0 * pi * m / nfft);
    }
}

}  // namespace fdt
