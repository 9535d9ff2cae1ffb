// dev_call.hpp — the device memory of ONE call: an entry point that needs device arrays for its own duration (the test hooks, the
// renderers, the ingest helpers, the k-mer counter, the batched queries) allocates them through a DevCall and never frees them
// itself.  What lives longer belongs to the handle: pool slots and OwnedBuf (pag_graph_impl.hpp).
#pragma once
#include <algorithm>
#include <vector>

#include "pag_device.hpp"

namespace pagdev {

struct DevCall {
    static constexpr int NO_STREAM = -1;
    const char *who = "";      // names the entry point in an out-of-memory message
    hipStream_t s = nullptr;   // what up / down / finish run on: open()'s own stream, or the one the caller put here (never destroyed)
    bool own_stream = false;
    int back = -1;             // the device to make current again
    std::vector<void *> bufs;
    explicit DevCall(const char *w = "") : who(w) {}
    DevCall(const DevCall &) = delete;
    DevCall &operator=(const DevCall &) = delete;
    // `device` current; restore_device: the caller's is put back when the scope ends; stream_flags: a stream of the call's own
    // (hipStreamDefault: blocking, hipStreamNonBlocking), NO_STREAM: s stays as it is
    int open(int device, bool restore_device, int stream_flags) {
        int before = -1;
        if (restore_device && hipGetDevice(&before) != hipSuccess) before = -1, (void)hipGetLastError();
        PAG_HIP_TRY(hipSetDevice(device));
        back = before == device ? -1 : before;
        if (stream_flags != NO_STREAM) {
            PAG_HIP_TRY(hipStreamCreateWithFlags(&s, (unsigned)stream_flags));
            own_stream = true;
        }
        return PAG_OK;
    }
    // n elements and `pad` bytes behind them (never an empty allocation), uninitialised
    template <typename T>
    int alloc(T **out, uint64_t n, size_t pad = 0) {
        const size_t bytes = std::max<size_t>(n * sizeof(T) + pad, 16);
        void *p = nullptr;
        const hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) {
            set_error("%s: hipMalloc(%zu) failed: %s", who, bytes, hipGetErrorString(e));
            return PAG_ENOMEM;
        }
        bufs.push_back(p);
        *out = (T *)p;
        return PAG_OK;
    }
    // ... filled with n elements of `host` (null or n == 0: nothing is copied), the `pad` bytes zeroed
    template <typename T>
    int up(const T *host, uint64_t n, T **out, size_t pad = 64) {
        const int rc = alloc(out, n, pad);
        if (rc) return rc;
        if (pad) PAG_HIP_TRY(hipMemsetAsync((char *)*out + n * sizeof(T), 0, pad, s));
        if (host && n) PAG_HIP_TRY(hipMemcpyAsync(*out, host, n * sizeof(T), hipMemcpyHostToDevice, s));
        return PAG_OK;
    }
    template <typename T>
    int down(T *host, const T *dev, uint64_t n) {
        if (n) PAG_HIP_TRY(hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, s));
        return PAG_OK;
    }
    int finish() {
        PAG_HIP_TRY(hipGetLastError());
        PAG_HIP_TRY(hipStreamSynchronize(s));
        return PAG_OK;
    }
    // the buffers given back early (the caller has waited for what used them)
    void release() {
        for (void *p : bufs) hipFree(p);
        bufs.clear();
    }
    ~DevCall() {
        if (own_stream || !bufs.empty()) (void)hipStreamSynchronize(s);
        release();
        if (own_stream) hipStreamDestroy(s);
        if (back >= 0) (void)hipSetDevice(back);
    }
};

}  // namespace pagdev
