// Ownership by type: DevBuf<T> owns one device allocation, HipOwner one HIP object (stream, event, graph exec, pinned buffer).
// All are move-only, release in their destructor and convert implicitly to the raw pointer / handle, so launch lines and
// `if (!h->x)` guards read as with raw pointers.  A struct made of them frees on every way out.  None may have static or
// thread-local storage duration: it would be destroyed after the HIP runtime has shut down.
// Pointers that are only borrowed stay raw and say so where they are declared: the kernel argument structs (GhostSrc, PutDst,
// AgPut / AgGet, PeerArgs, TimeTerm::d and ::nu_t, LpMat), a plan's places in its communicator's window, the caller's stream.
// DevBuf needs no HIP header (csrc/sns_internal.h is compiled by g++ too); the HIP owners exist under hipcc only.
#pragma once
#include <cstddef>
#include <type_traits>
#include <vector>

#include "sns.h"

namespace sns {

// The allocator behind every DevBuf, defined once in the library (csrc/sns_api.hip, over hipMalloc / hipFree / hipMemcpy; a host
// test supplies its own).  They keep the count of live bytes that sns_live_device_bytes() returns.  dev_malloc_bytes: SNS_OK, or
// SNS_E_HIP with the error text set and *p null.
int dev_malloc_bytes(void** p, size_t bytes);
void dev_free_bytes(void* p, size_t bytes);
int dev_upload_bytes(void* dst, const void* src, size_t bytes);

template <class T>
class DevBuf {                                   // (DevBuf<void>: a byte buffer)
    static constexpr size_t ELEM = sizeof(std::conditional_t<std::is_void<T>::value, char, T>);
    T* p_ = nullptr;
    size_t n_ = 0;

public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_; n_ = o.n_;
            o.p_ = nullptr; o.n_ = 0;
        }
        return *this;
    }
    ~DevBuf() { reset(); }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t count() const { return n_; }
    void reset() {
        if (p_) dev_free_bytes(p_, n_ * ELEM);
        p_ = nullptr;
        n_ = 0;
    }
    // frees what it holds; 0 means 1 element (a kernel argument is never a null pointer)
    int alloc(size_t count) {
        reset();
        if (count == 0) count = 1;
        void* q = nullptr;
        const int rc = dev_malloc_bytes(&q, count * ELEM);
        if (rc != SNS_OK) return rc;
        p_ = static_cast<T*>(q);
        n_ = count;
        return SNS_OK;
    }
    template <class U = T>
    int upload(const std::vector<U>& v) {
        static_assert(std::is_same<U, T>::value, "upload: element type");
        const int rc = alloc(v.size());
        if (rc != SNS_OK || v.empty()) return rc;
        return dev_upload_bytes(p_, v.data(), v.size() * ELEM);
    }
};

}  // namespace sns

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace sns {

// one HIP object of handle type H, destroyed by Destroy.  put(): the address for the create call (releases what it holds first)
template <class H, hipError_t (*Destroy)(H)>
class HipOwner {
    H h_ = nullptr;

public:
    HipOwner() = default;
    HipOwner(const HipOwner&) = delete;
    HipOwner& operator=(const HipOwner&) = delete;
    HipOwner(HipOwner&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    HipOwner& operator=(HipOwner&& o) noexcept {
        if (this != &o) { reset(); h_ = o.h_; o.h_ = nullptr; }
        return *this;
    }
    ~HipOwner() { reset(); }
    void reset() {
        if (h_) (void)Destroy(h_);
        h_ = nullptr;
    }
    operator H() const { return h_; }
    H* put() { reset(); return &h_; }
};

inline hipError_t pinned_free(double* p) { return hipHostFree(p); }

using Stream = HipOwner<hipStream_t, hipStreamDestroy>;
using Event = HipOwner<hipEvent_t, hipEventDestroy>;
using GraphExec = HipOwner<hipGraphExec_t, hipGraphExecDestroy>;
using PinnedDoubles = HipOwner<double*, pinned_free>;

}  // namespace sns
#endif
