// art_own.h -- the owning handles of libart's host side: device memory, pinned memory, events and streams.  Each is move-only, owns nothing by default and releases
// what it holds in its destructor; each is the pointer it replaces (`p`) and converts to it.  Together with the stream pool of art_api.hip these are the only callers
// of the HIP allocation, event-creation and stream-creation functions in libart, so the counts behind art_parity_live_resources cannot miss one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>

#pragma GCC visibility push(hidden)
namespace art {
// what libart holds in this process right now (art_parity_live_resources, include/art_parity.h): relaxed counters, bumped where a handle acquires or releases
enum Live { kLiveDevice = 0, kLivePinned = 1, kLiveEvents = 2, kLiveStreams = 3, kLivePooled = 4 };
inline std::atomic<uint64_t> g_live[5];
inline void live_add(Live what, int64_t d) { g_live[what].fetch_add((uint64_t)d, std::memory_order_relaxed); }
template <class H> hipError_t acquired(hipError_t r, H &p, Live what) { if (r == hipSuccess) live_add(what, 1); else p = H{}; return r; }   // the tail of every acquire below

template <class H, void (*Drop)(H)> struct Owned {   // the one raw handle p, released by Drop
    H p{};
    Owned() = default;
    Owned(Owned &&o) noexcept : p(o.p) { o.p = H{}; }
    Owned &operator=(Owned &&o) noexcept { if (this != &o) { release(); p = o.p; o.p = H{}; } return *this; }
    ~Owned() { release(); }
    operator H() const { return p; }
    void release() { if (p) Drop(p); p = H{}; }
};
template <class T> void drop_device(T *p) { (void)hipFree(p); live_add(kLiveDevice, -1); }
template <class T> void drop_pinned(T *p) { (void)hipHostFree(p); live_add(kLivePinned, -1); }
inline void drop_event(hipEvent_t e) { (void)hipEventDestroy(e); live_add(kLiveEvents, -1); }
inline void drop_stream(hipStream_t s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); live_add(kLiveStreams, -1); }   // (waited for before it goes)

// device memory: n elements at p.  ensure() only grows (the old contents go); n means something only while p is set
template <class T> struct DevBuf : Owned<T *, drop_device<T>> {
    size_t n = 0;
    hipError_t ensure(size_t count) {
        if (count <= n && this->p) return hipSuccess;
        this->release(); n = count ? count : 1;
        return acquired(hipMalloc(&this->p, n * sizeof(T)), this->p, kLiveDevice);
    }
};
// pinned host memory the device reads and writes in place: n elements at p, which the device sees at d
template <class T> struct Pinned : Owned<T *, drop_pinned<T>> {
    T *d = nullptr; size_t n = 0;
    hipError_t ensure(size_t count) {
        if (count <= n && this->p) return hipSuccess;
        this->release(); n = count ? count : 1;
        hipError_t e = acquired(hipHostMalloc((void **)&this->p, n * sizeof(T), hipHostMallocDefault), this->p, kLivePinned);
        if (e == hipSuccess && (e = hipHostGetDevicePointer((void **)&d, this->p, 0)) != hipSuccess) this->release();
        return e;
    }
};
// an event: create() makes it once (a pointer compare from then on), with the flags given
struct Event : Owned<hipEvent_t, drop_event> {
    hipError_t create(unsigned flags = hipEventDefault) { return p ? hipSuccess : acquired(hipEventCreateWithFlags(&p, flags), p, kLiveEvents); }
};
// a stream its owner creates and destroys itself (the refit streams, the wave plan's, the exchange's): non-blocking, made once
struct Stream : Owned<hipStream_t, drop_stream> {
    hipError_t create() { return p ? hipSuccess : acquired(hipStreamCreateWithFlags(&p, hipStreamNonBlocking), p, kLiveStreams); }
    hipError_t create(int priority) { return p ? hipSuccess : acquired(hipStreamCreateWithPriority(&p, hipStreamNonBlocking, priority), p, kLiveStreams); }
};
// Frame and cast streams come from a pool kept for the life of the process (art_api.hip says why): the pool is the only place that creates them, and counts them
hipError_t acquire_stream(int device, hipStream_t *out);
void release_stream(int device, hipStream_t s);   // waits for the stream, then parks it
struct PoolStream {
    hipStream_t p = nullptr; int device = 0;
    PoolStream() = default; PoolStream(const PoolStream &) = delete;
    ~PoolStream() { if (p) release_stream(device, p); }
    operator hipStream_t() const { return p; }
    hipError_t acquire(int dev) { device = dev; return p ? hipSuccess : acquire_stream(dev, &p); }
};
} // namespace art
#pragma GCC visibility pop
