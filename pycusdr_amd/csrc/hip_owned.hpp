// hip_owned.hpp -- move-only owners of what mfbank.hip used to free by hand: device memory, page-locked host memory, events,
// and the streams the library creates itself.  Host code only.
//
// Each owner is a std::unique_ptr with the matching destroy call as its deleter, inside a class this thin:
//   * it converts to the raw pointer / handle, so launches, copies, pointer arithmetic and null tests read as with raw pointers
//     (casts that reinterpret, `(BlockScalars *)buf`, take .get());
//   * reset() RETURNS what the destroy call said: a reserve path reports a failing hipFree (HIPCHK), a destructor ignores it,
//     as teardown always has.  The owner is empty afterwards either way;
//   * alloc() goes through an allocation function of the caller's choice -- a handle's device memory through dev_alloc
//     (mfb_debug_fail_alloc), everything else through hip_malloc / hip_host_malloc below.
#pragma once
#include <hip/hip_runtime.h>
#include <memory>
#include <type_traits>

struct DevFree {
    static hipError_t destroy(void *p) noexcept { return hipFree(p); }
    void operator()(void *p) const noexcept { (void)destroy(p); }
};
struct HostFree {
    static hipError_t destroy(void *p) noexcept { return hipHostFree(p); }
    void operator()(void *p) const noexcept { (void)destroy(p); }
};
struct EventDestroy {
    static hipError_t destroy(void *p) noexcept { return hipEventDestroy((hipEvent_t)p); }
    void operator()(void *p) const noexcept { (void)destroy(p); }
};
struct StreamDestroy {
    static hipError_t destroy(void *p) noexcept { return hipStreamDestroy((hipStream_t)p); }
    void operator()(void *p) const noexcept { (void)destroy(p); }
};

using AllocFn = hipError_t (*)(void **, size_t);
inline hipError_t hip_malloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
inline hipError_t hip_host_malloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
// ... for memory the host reads while the kernel that writes it still runs
inline hipError_t hip_host_malloc_coherent(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocCoherent); }

// The untyped part (what a group of buffers of different element types has in common: grow_buffers in bank_ctx.hpp).
template <class Del>
class Mem {
    std::unique_ptr<void, Del> p_;

public:
    void *get() const noexcept { return p_.get(); }
    // destroy what is held, take over `fresh`
    hipError_t reset(void *fresh = nullptr) noexcept {
        void *old = p_.release();
        p_.reset(fresh);
        return old ? Del::destroy(old) : hipSuccess;
    }
    // destroy what is held, then `bytes` from `fn`: empty unless that succeeded
    hipError_t alloc(size_t bytes, AllocFn fn) {
        hipError_t e = reset();
        if (e != hipSuccess) return e;
        void *p = nullptr;
        if ((e = fn(&p, bytes)) == hipSuccess) p_.reset(p);
        return e;
    }
};
template <class T, class Del>
struct Owned : Mem<Del> {
    using pointer = T *;
    T *get() const noexcept { return static_cast<T *>(Mem<Del>::get()); }
    operator T *() const noexcept { return get(); }
    T *operator->() const noexcept { return get(); }
};
template <class T>
using DevBuf = Owned<T, DevFree>;
template <class T>
using HostBuf = Owned<T, HostFree>;
using Event = Owned<std::remove_pointer_t<hipEvent_t>, EventDestroy>;
using Stream = Owned<std::remove_pointer_t<hipStream_t>, StreamDestroy>;

// For the create calls that answer through a pointer -- hipEventCreate(out(e)), hipStreamCreateWithPriority(out(s), ...): what they
// wrote is the owner's when the full expression ends.
template <class O>
class Out {
    O &o_;
    typename O::pointer p_ = nullptr;

public:
    explicit Out(O &o) : o_(o) {}
    ~Out() {
        if (p_) (void)o_.reset(p_);
    }
    operator typename O::pointer *() noexcept { return &p_; }
};
template <class O>
Out<O> out(O &o) { return Out<O>(o); }

// The bookkeeping half of a grow-only buffer: too small -> destroyed; the owner empty and the capacity 0 until the new allocation
// has succeeded; then the capacity.  What has to be waited for first, and whether recorded graphs die with the old address, is the
// caller's business, BEFORE the call.
template <class Del, class Cap>
hipError_t reserve(Mem<Del> &m, Cap &cap, Cap want, size_t bytes, AllocFn fn) {
    if (m.get() && cap >= want) return hipSuccess;
    cap = 0;
    const hipError_t e = m.alloc(bytes, fn);
    if (e == hipSuccess) cap = want;
    return e;
}

static_assert(!std::is_copy_constructible<DevBuf<float>>::value && !std::is_copy_assignable<DevBuf<float>>::value, "owners do not copy");
static_assert(!std::is_copy_constructible<HostBuf<float>>::value && !std::is_copy_constructible<Event>::value &&
                  !std::is_copy_constructible<Stream>::value, "owners do not copy");
static_assert(std::is_nothrow_move_constructible<DevBuf<float>>::value && std::is_nothrow_move_assignable<DevBuf<float>>::value &&
                  std::is_nothrow_move_constructible<HostBuf<float>>::value && std::is_nothrow_move_assignable<HostBuf<float>>::value &&
                  std::is_nothrow_move_constructible<Event>::value && std::is_nothrow_move_assignable<Event>::value &&
                  std::is_nothrow_move_constructible<Stream>::value && std::is_nothrow_move_assignable<Stream>::value,
              "owners move without throwing (std::vector<Event>)");
