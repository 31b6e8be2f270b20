// ise_host.hpp -- host plumbing every translation unit of libise_knn.so shares: the error path into
// ise_last_error(), the device gate of every *_create, the lazily grown buffer (device or page-locked) with every grow
// rule of the library, the call order of a handle with ONE set of workspaces and the hand-out of workspace slots, the
// non-finite flag of the encoders, the kNN argument checks and the small helpers, and the one knob another translation
// unit reads.  Plain structs and inline functions; no kernels.
#pragma once
#include "ise_common.hpp"

// ise_knn.hip: stores msg as the calling thread's ise_last_error() and returns code
int ise_fail_(int code, const std::string& msg);
// ise_knn.hip: $ISE_REMOVE_SLAB_ROWS as last refreshed (ise_refresh_env_knobs)
int ise_remove_slab_rows_();

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return ise_fail_(e_ == hipErrorOutOfMemory ? ISE_E_NOMEM : ISE_E_HIP,                  \
                             std::string(#expr) + ": " + hipGetErrorString(e_));                   \
    } while (0)

// ---- the device gate: what every *_create asks of `device` before it allocates anything.  *num_cu: its compute units
inline int device_gate(int device, int* num_cu) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return ise_fail_(ISE_E_NODEVICE, "no HIP device visible: the kNN path needs an MI355X (gfx950) GPU");
    if (device < 0 || device >= ndev) return ise_fail_(ISE_E_INVALID, "device out of range");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return ise_fail_(ISE_E_NODEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    *num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    return ISE_OK;
}

// ---- a buffer grown lazily, contents not kept: device memory, page-locked host memory, or page-locked host memory
// the device addresses too (`dev`).  buf_realloc is the one way such a buffer comes to hold memory and buf_free the one
// way it lets go of it; what decides a replacement is a grow rule below.  Each rule answers three questions: is the
// buffer already enough, what is waited for before the free, and how much is asked for.  A handle's kind picks its
// rule; the rules block differently, so each stays a function of its own.
enum MemKind { MEM_DEVICE, MEM_PINNED, MEM_MAPPED };
template <class T, MemKind K = MEM_DEVICE>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
};
template <class T>
struct DevBuf<T, MEM_MAPPED> {
    T* p = nullptr;
    size_t n = 0;
    T* dev = nullptr;  // p as the device addresses it
};

template <class T, MemKind K>
void buf_free(DevBuf<T, K>& b) {
    if (b.p) (void)(K == MEM_DEVICE ? hipFree(b.p) : hipHostFree(b.p));
    b = DevBuf<T, K>();
}
template <class... B>
void buf_free(B&... b) {
    (buf_free(b), ...);
}
// frees what b holds, allocates `want` elements and records the size
template <class T, MemKind K>
int buf_realloc(DevBuf<T, K>& b, size_t want) {
    buf_free(b);
    if constexpr (K == MEM_DEVICE) HIP_TRY(hipMalloc((void**)&b.p, want * sizeof(T)));
    else HIP_TRY(hipHostMalloc((void**)&b.p, want * sizeof(T), K == MEM_MAPPED ? hipHostMallocMapped : hipHostMallocDefault));
    if constexpr (K == MEM_MAPPED) HIP_TRY(hipHostGetDevicePointer((void**)&b.dev, b.p, 0));
    b.n = want;
    return ISE_OK;
}

// rule: device-wide drain before a free (any stream may still use the handle's ONE set), and half again on top so growth drains rarely
template <class T>
int grow_drained(DevBuf<T>& b, size_t need) {
    if (b.p && need <= b.n) return ISE_OK;
    if (b.p) HIP_TRY(hipDeviceSynchronize());  // work in flight on any stream may still use the old one
    return buf_realloc(b, std::max<size_t>(need + need / 2, 16));
}

// rule: device-wide drain before a free (work in flight on any stream may still use the handle's ONE set); exact size
template <class T>
int grow_drained_exact(DevBuf<T>& b, size_t need) {
    if (b.p && need <= b.n) return ISE_OK;
    if (b.p) HIP_TRY(hipDeviceSynchronize());
    return buf_realloc(b, std::max<size_t>(need, 16));
}

// busy: the event behind the last pass that used the workspaces (CallOrder::busy), or null -- waited for only when the
// buffer really has to be replaced (then the call blocks)
// rule: a free waits for that one event only -- every pass that used the workspaces is ordered before it; exact size
template <class T>
int grow_after_event(DevBuf<T>& b, size_t need, hipEvent_t busy) {
    if (need <= b.n) return ISE_OK;
    if (b.p && busy) HIP_TRY(hipEventSynchronize(busy));
    return buf_realloc(b, need);
}

// rule: no wait before a free -- range search owns its workspace (rg_mu) and drains it per batch, a SelSlot's other user was waited for, a host context is its caller's; exact size, `floor` at least
template <class T, MemKind K>
int grow_owned(DevBuf<T, K>& b, size_t need, size_t floor = 1) {
    if (b.p && need <= b.n) return ISE_OK;
    return buf_realloc(b, std::max(need, floor));
}

// rule: no wait of its own -- hipFree waits for outstanding work; exact size; *changed: something was allocated (the caller fills and drains once)
template <class T>
int grow_slot(DevBuf<T>& b, size_t need, bool* changed) {
    if (need <= b.n) return ISE_OK;
    *changed = true;
    return buf_realloc(b, need);
}

// ---- the call order of a handle with ONE set of workspaces (its mutex held): device work enqueued on another stream
// than the previous call's waits for that call through an event.  Where a call waits and where it marks its end is the
// call site's business; the inverted-list kinds mark through a Scope, on every return path once a pass may be enqueued.
struct CallOrder {
    hipEvent_t ev = nullptr;  // the end of the previous call's device work
    hipStream_t last_stream = nullptr;
    bool valid = false;

    hipError_t create() { return hipEventCreateWithFlags(&ev, hipEventDisableTiming); }
    void destroy() {
        if (ev) (void)hipEventDestroy(ev);
        ev = nullptr;
    }
    // order st's work from here on behind the previous call's
    int wait(hipStream_t st) {
        if (valid && last_stream != st) HIP_TRY(hipStreamWaitEvent(st, ev, 0));
        return ISE_OK;
    }
    // mark this call's end on st
    int mark(hipStream_t st) {
        HIP_TRY(hipEventRecord(ev, st));
        last_stream = st;
        valid = true;
        return ISE_OK;
    }
    // the device has drained: nothing to order the next call behind
    void forget() { valid = false; }
    // what grow_after_event waits for
    hipEvent_t busy() const { return valid ? ev : nullptr; }

    struct Scope {  // whatever path returns, a later user on another stream waits for this call
        CallOrder& o;
        hipStream_t st;
        ~Scope() {
            if (hipEventRecord(o.ev, st) == hipSuccess) { o.valid = true; o.last_stream = st; }
        }
    };
};

// ---- slots of workspaces, each with a CallOrder `order` (the handle's mutex held): a stream keeps the slot it used
// last (stream order is all the ordering that needs); a stream without one takes a fresh slot, or the least recently
// taken one behind an event wait.  *waited (optional): the slot's last user was another stream.  The caller marks the
// slot's end through a CallOrder::Scope
template <class Slot, int N>
int take_slot(Slot (&slots)[N], unsigned* next, hipStream_t st, Slot** out, bool* waited) {
    Slot* w = nullptr;
    for (auto& s : slots)
        if (s.order.valid && s.order.last_stream == st) { w = &s; break; }
    if (!w)
        for (auto& s : slots)
            if (!s.order.valid) { w = &s; break; }
    if (!w) w = &slots[(*next)++ % N];
    if (waited) *waited = w->order.valid && w->order.last_stream != st;
    *out = w;
    return w->order.wait(st);
}

// ---- the encoders' non-finite flag: [1] on the device, set by an encode that met a NaN or inf entry
struct BadFlag {
    unsigned int* p = nullptr;

    hipError_t create() { return hipMalloc((void**)&p, sizeof(unsigned int)); }
    int clear(hipStream_t st) {
        HIP_TRY(hipMemsetAsync(p, 0, sizeof(unsigned int), st));
        return ISE_OK;
    }
    // waits for st; ISE_E_INVALID when an encode since clear met a non-finite entry
    int check(hipStream_t st) {
        unsigned int flag = 0;
        HIP_TRY(hipMemcpyAsync(&flag, p, sizeof(flag), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return flag ? ise_fail_(ISE_E_INVALID, "a row has a NaN or inf entry: nothing was encoded or added") : ISE_OK;
    }
};

// ---- small helpers
// rows of `step` at most so that one upload is 256 MiB at most
inline long long upload_step(size_t row_bytes) { return std::max<long long>(1, (1ll << 28) / (long long)row_bytes); }

// the arguments of a kNN search, host or device form
inline int check_knn_args(const void* q, long long nq, int k, const void* D, const void* I) {
    if (nq < 0) return ise_fail_(ISE_E_INVALID, "nq must be >= 0");
    if (k < 1 || k > ISE_MAX_K) return ise_fail_(ISE_E_INVALID, "k must be in [1, ISE_MAX_K]");
    if (nq > 0 && !q) return ise_fail_(ISE_E_INVALID, "query pointer is NULL");
    if (nq > 0 && (!D || !I)) return ise_fail_(ISE_E_INVALID, "output pointer is NULL");
    if (nq * (long long)k >= (1ll << 40)) return ise_fail_(ISE_E_INVALID, "nq * k is too large");
    return ISE_OK;
}

// device allocations of a scope's duration: what the listed pointers hold when it ends is freed (null: nothing)
template <size_t N>
struct DevFreeList {
    void** p[N];
    ~DevFreeList() {
        for (void** q : p)
            if (*q) (void)hipFree(*q);
    }
};
