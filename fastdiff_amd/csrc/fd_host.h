// fd_host.h -- shared by the host translation units of libfastdiff_hip.so (fd_api.cpp, fd_weights.cpp, fd_api_ext.cpp, fd_api_span.cpp,
// fd_api_train.cpp): the error macros and the few helpers of the core that the others call.
#pragma once
#include <stdio.h>

#include <string>

#include "fd_internal.h"

extern std::string g_create_error;      // text of a failed fd_create (no handle to keep it)

#define FD_FAIL(h, code, ...)                                   \
    do {                                                        \
        char buf__[512];                                        \
        snprintf(buf__, sizeof(buf__), __VA_ARGS__);            \
        if (h) (h)->err = buf__; else g_create_error = buf__;   \
        return (code);                                          \
    } while (0)

#define FD_HIP(h, expr)                                                                                   \
    do {                                                                                                  \
        hipError_t e__ = (expr);                                                                          \
        if (e__ != hipSuccess) FD_FAIL(h, FD_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e__));    \
    } while (0)

extern "C" {      // (defined inside fd_api.cpp's extern "C" block; hidden visibility: not part of the ABI)
// fallback = host: look at the flags of a pending fd_sample before touching device state (no-op when nothing is pending)
int fd_settle(fd_handle h);
// the range flags of a pending fd_refresh_weights_device (fd_weights.cpp): waits for that refresh alone; a flag that changed drops the
// graphs.  Every inference entry point calls it before it chooses a kernel family (no-op when nothing is pending)
int fd_settle_refresh(fd_handle h);
// drops every captured graph; the caller has synchronised the device
void drop_graph(fd_context *c);
// Pinned staging ring (fd_context::stage): the next slot with room for `bytes`, free to be written by the host; ... and the mark behind
// the copies that read it
int fd_stage_acquire(fd_handle h, size_t bytes, fd_context::StageSlot **out);
int fd_stage_commit(fd_handle h, fd_context::StageSlot *sl, hipStream_t stream);
// host bytes -> the device array `dev` through one slot of that ring (the call does not wait for the copy)
int fd_stage_upload(fd_handle h, const void *src, size_t bytes, void *dev, hipStream_t stream);
// one stream at a time per handle: a call on another stream first waits for the tail of the handle's last call; ... and the tail's mark
int fd_follow_stream(fd_handle h, hipStream_t s);
int fd_mark_tail(fd_handle h, hipStream_t s);
}
void fd_prof_drain(fd_context *c);

static bool capturing(hipStream_t stream)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone) return false;
    (void)hipGetLastError();
    return true;
}

// A scratch buffer of the handle holds at least `need` bytes: grown at the first call that needs more (hipFree waits for the calls that
// still use the old one), never inside a capture, whose graph would keep the old pointers.  Calls on one handle share these buffers:
// they must be ordered on one stream, as torch.autograd orders a forward and its backward.
static int reserve(fd_handle h, const char *who, Scratch &s, size_t need, hipStream_t stream)
{
    if (s.bytes >= need) return FD_OK;
    if (capturing(stream))
        FD_FAIL(h, FD_ERR_STATE, "%s: the scratch buffer has to grow to %zu bytes, which cannot happen inside a stream capture: call it once before", who, need);
    FD_HIP(h, hipSetDevice(h->device));
    if (s.p) FD_HIP(h, hipFree(s.p));
    s = Scratch{};
    void *p = nullptr;
    FD_HIP(h, hipMalloc(&p, need));
    s.p = static_cast<float *>(p);
    s.bytes = need;
    return FD_OK;
}

// What an entry point ends with once its arguments are checked: the handle's device, one Launch on `stream`, and a failure of
// `launch` reported as "<who>: <HIP error>".
template <class F>
static int run(fd_handle h, void *stream, const char *who, F &&launch)
{
    FD_HIP(h, hipSetDevice(h->device));
    const hipError_t e = launch(fdk::Launch{h, (hipStream_t)stream, false});
    if (e != hipSuccess) FD_FAIL(h, FD_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return FD_OK;
}

// ... with `floats` floats of scratch `s` reserved first: launch(L, s.p)
template <class F>
static int run_scratch(fd_handle h, void *stream, const char *who, Scratch &s, size_t floats, F &&launch)
{
    const int rc = reserve(h, who, s, sizeof(float) * floats, (hipStream_t)stream);
    return rc != FD_OK ? rc : run(h, stream, who, [&](const fdk::Launch &L) { return launch(L, s.p); });
}
