// mdk_side.hpp -- the host layer the side libraries share (libmdk_index/stats/track/smooth/cohort.so: one .hip file, one code object, one
// .so each, loaded at the first call that needs it).  Host code only, everything static: a library includes this below its kernels and
// holds a copy of its own, so none of them links to another.  Before the include a library names its three return codes:
//   #define SIDE_ERR_ARG / SIDE_ERR_HIP / SIDE_ERR_NOMEM   (MD_X_ERR_* of its header)
// and it exports `extern "C" const char *md_X_last_error(void) { return g_err; }` itself.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>

// ---- errors: the calling thread's text, and the return code that goes with it ----
static thread_local char g_err[512];
static int fail(int rc, const char *what, hipError_t e) {
    if(e != hipSuccess) snprintf(g_err, sizeof g_err, "%s: %s", what, hipGetErrorString(e)); else snprintf(g_err, sizeof g_err, "%s", what);
    return rc;
}
// (the text of a failed call is the call as its library spells it: a macro, and so are the two below that make calls for a library)
#define SIDECHK(x) do { const hipError_t e_ = (x); if(e_ != hipSuccess) return fail(SIDE_ERR_HIP, #x, e_); } while(0)

// ---- a buffer that is kept and grows: device memory, or (`pinned`) host memory the device copies to and from ----
template <typename T, bool pinned = false> struct SideBuf {
    T *p = nullptr; size_t cap = 0;
    operator T *() const { return p; }
    // room for n entries.  A buffer too small is released and one of `room` >= n entries takes its place: how far past n is the caller's policy
    int need(size_t n, size_t room, const char *what) {
        if(n <= cap) return 0;
        release();
        const hipError_t e = pinned ? hipHostMalloc((void **)&p, room * sizeof(T), hipHostMallocDefault) : hipMalloc((void **)&p, room * sizeof(T));
        if(e != hipSuccess) { p = nullptr; return fail(SIDE_ERR_NOMEM, what, e); }
        cap = room; return 0;
    }
    int need(size_t n, const char *what) { return need(n, n, what); }          // an exact fit
    void release() { if(p) (void)(pinned ? hipHostFree(p) : hipFree(p)); p = nullptr; cap = 0; }
};

// ---- a handle's device and a stream of its own on it (md_index has these alone: it is opened per file, with a status of its own) ----
struct SideStream {
    int device = 0; hipStream_t st = nullptr;
    hipError_t open(int device_) {                              // (after hipSetDevice(device_))
        device = device_;
        return hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    }
    void close() {                                              // what lies on the device is released behind this: the device is the handle's by then
        (void)hipSetDevice(device);
        if(st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    }
};

// ---- what a handle of stats, smooth, track and cohort starts with: the kernels' status word beside them, and a pinned mirror of it
// (Mirror: Status itself, or a struct that holds more beside it) ----
template <typename Status, typename Mirror = Status> struct SideHandle : SideStream {
    Status *d_st = nullptr; Mirror *pin = nullptr;
    hipError_t open(int device_) {
        hipError_t e = SideStream::open(device_);
        if(e == hipSuccess) e = hipMalloc((void **)&d_st, sizeof(Status));
        if(e == hipSuccess) e = hipHostMalloc((void **)&pin, sizeof(Mirror), hipHostMallocDefault);
        return e;
    }
    void close() {
        SideStream::close();
        (void)hipFree(d_st);
        if(pin) (void)hipHostFree(pin);
    }
};

// md_X_open: the base's part, then `more(h)` -- what the library allocates beside it, a hipError_t --; a failure closes what was opened
template <typename H, typename More> static int side_open(int device, H **out, const char *what, void (*close)(H *), More more) {
    if(!out) return fail(SIDE_ERR_ARG, what, hipSuccess);
    *out = nullptr;
    SIDECHK(hipSetDevice(device));
    H *h = new H();
    hipError_t e = h->open(device);
    if(e == hipSuccess) e = more(h);
    if(e != hipSuccess) { close(h); return fail(SIDE_ERR_NOMEM, what, e); }
    *out = h;
    return 0;
}
template <typename H> static int side_open(int device, H **out, const char *what, void (*close)(H *)) {
    return side_open(device, out, what, close, [](H *) { return hipSuccess; });
}

// status up: `first` all ones in the mirror (h->pin, or the status inside it) and the mirror on its way to the device;
// status down: the device's word on its way back and the stream waited for.  `first` is decoded where it is read: every library packs its own
#define SIDE_STATUS_UP(h, mirror, Status) do { (mirror)->first = ~0ull; SIDECHK(hipMemcpyAsync(h->d_st, mirror, sizeof(Status), hipMemcpyHostToDevice, h->st)); } while(0)
#define SIDE_STATUS_DOWN(h, mirror, Status) do { SIDECHK(hipMemcpyAsync(mirror, h->d_st, sizeof(Status), hipMemcpyDeviceToHost, h->st)); SIDECHK(hipStreamSynchronize(h->st)); } while(0)
