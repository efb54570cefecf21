/* hip_owned.h — move-only owners of the engine's HIP objects (engine.hip): stream, event, device and pinned host allocation (Staged: a ring of two).  An owner
 * releases its object when it goes or is reset, and nothing else in the engine does (tests/test_abi.py); waiting for the device first is
 * the holder's business.  A creation that fails leaves the owner empty and returns the HIP error. */
#ifndef H264BSD_AMD_HIP_OWNED_H
#define H264BSD_AMD_HIP_OWNED_H
#include <hip/hip_runtime.h>
#include <algorithm>
#include <utility>

void tickets_release(hipStream_t st);       /* engine.hip: the ticket counters of the stream's banded launches */

template <class H, void (*Release)(H)> class Owned {
public:
    Owned() = default;
    Owned(Owned &&o) noexcept : h_(std::exchange(o.h_, H())) {}
    Owned &operator=(Owned &&o) noexcept { if (this != &o) { reset(); h_ = std::exchange(o.h_, H()); } return *this; }
    ~Owned() { reset(); }
    void reset() { if (h_) Release(std::exchange(h_, H())); }
    operator H() const { return h_; }
    H get() const { return h_; }
protected:
    H h_ = H();
    hipError_t created(hipError_t err) { if (err != hipSuccess) h_ = H(); return err; }
};
inline void stream_destroy(hipStream_t s) { tickets_release(s); (void)hipStreamDestroy(s); }
inline void event_destroy(hipEvent_t ev) { (void)hipEventDestroy(ev); }
template <class T> void device_free(T *p) { (void)hipFree(p); }
template <class T> void host_free(T *p) { (void)hipHostFree(p); }

struct Stream : Owned<hipStream_t, stream_destroy> {      /* non-blocking; high: created with a priority of its own */
    bool high = false;
    hipError_t create() { reset(); high = false; return created(hipStreamCreateWithFlags(&h_, hipStreamNonBlocking)); }
    hipError_t create(int priority) { reset(); high = true; return created(hipStreamCreateWithPriority(&h_, hipStreamNonBlocking, priority)); }
};
struct Event : Owned<hipEvent_t, event_destroy> {
    hipError_t create(unsigned flags = hipEventDefault) { reset(); return created(hipEventCreateWithFlags(&h_, flags)); }
};
template <class T> struct DeviceMem : Owned<T *, device_free<T>> {
    hipError_t alloc(size_t bytes) { this->reset(); return this->created(hipMalloc((void **)&this->h_, bytes)); }
};
/* pinned host memory; dev(): the device's address of it, where alloc() was asked for one */
template <class T> struct Pinned : Owned<T *, host_free<T>> {
    hipError_t alloc(size_t bytes, bool with_dev = false)
    {
        this->reset(); d_ = nullptr;
        hipError_t err = this->created(hipHostMalloc((void **)&this->h_, bytes, hipHostMallocDefault));
        if (err == hipSuccess && with_dev && (err = hipHostGetDevicePointer((void **)&d_, this->h_, 0)) != hipSuccess) this->reset();
        return err;
    }
    T *dev() const { return this->h_ ? d_ : nullptr; }
private:
    T *d_ = nullptr;
};
/* Pinned staging that launches read while the host fills the next one's: two halves of cap() elements used in turn, each guarded by an
 * event recorded behind the launch that read it.  A half is free when nothing was submitted from it yet or its event has passed — with
 * two halves, the launch before the last one read it.  Per use: reserve(), fill host(), launch with dev(), submit() on that stream. */
template <class T> class Staged {
public:
    /* room for n elements in the current half, and that half free; a ring that is too small waits for the readers of both halves, is
     * allocated again with max(n, min_cap) elements per half and starts over at half 0 */
    hipError_t reserve(size_t n, size_t min_cap = 0)
    {
        hipError_t err;
        if (n > cap_) {
            for (int k = 0; k < 2; k++)
                if (used_[k] && (err = hipEventSynchronize(ev_[k])) != hipSuccess) return err;
            cap_ = 0; cur_ = 0; used_[0] = used_[1] = false;
            if ((err = mem_.alloc(2 * std::max(n, min_cap) * sizeof(T), true)) != hipSuccess) return err;
            for (Event &ev : ev_)
                if (!ev && (err = ev.create(hipEventDisableTiming)) != hipSuccess) return err;
            cap_ = std::max(n, min_cap);
        }
        return used_[cur_] ? hipEventSynchronize(ev_[cur_]) : hipSuccess;
    }
    /* the current half as the host fills it / as the device reads it (U: what the elements hold); half(): for a buffer kept beside the ring under its guard */
    template <class U = T> U *host() const { return reinterpret_cast<U *>(mem_.get() + (size_t)cur_ * cap_); }
    template <class U = T> const U *dev() const { return reinterpret_cast<const U *>(mem_.dev() + (size_t)cur_ * cap_); }
    size_t cap() const { return cap_; }    int half() const { return cur_; }
    /* the launch that reads the current half is on st: guard the half, go on to the other */
    hipError_t submit(hipStream_t st)
    {
        const hipError_t err = hipEventRecord(ev_[cur_], st);
        if (err == hipSuccess) { used_[cur_] = true; cur_ ^= 1; }
        return err;
    }
private:
    Pinned<T> mem_; Event ev_[2]; bool used_[2] = { false, false };
    size_t cap_ = 0; int cur_ = 0;
};
#endif
