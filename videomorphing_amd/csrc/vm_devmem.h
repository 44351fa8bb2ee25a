// vm_devmem.h -- owners of the host side's device buffers, pinned host buffers and HIP events.
// Every hipMalloc / hipHostMalloc / hipEventCreate of the C-ABI implementation goes through these
// types; their destructors free.  A buffer is freed on whatever device is current, so its owner
// is destroyed with the owning device current (vm_destroy_object, vm_host.h).
#ifndef VM_DEVMEM_H
#define VM_DEVMEM_H

#include <hip/hip_runtime.h>
#include <cstddef>
#include "../../include/vmorph.h"

int vm_fail(int code, const char *fmt, ...);

// arrays carved from one allocation each start on a 256-byte boundary
inline size_t vm_align256(size_t b) { return (b + 255) & ~(size_t)255; }

enum class VmMem { Device, Pinned };

// One allocation of `capacity()` elements of T: device memory (hipMalloc) or pinned host memory (hipHostMalloc).
template <class T, VmMem K>
class VmBuf {
public:
    VmBuf() = default;
    VmBuf(VmBuf &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    VmBuf(const VmBuf &) = delete;
    VmBuf &operator=(const VmBuf &) = delete;
    ~VmBuf() { reset(); }

    T *get() const { return p_; }
    size_t capacity() const { return n_; }

    // Grow only: reallocates (contents not kept) when n exceeds the capacity, after draining drain_stream if one is
    // given.  A failed allocation leaves the buffer empty; a failed drain leaves it as it was (it may still be in use).
    int reserve(size_t n, hipStream_t drain_stream = nullptr)
    {
        if (n <= n_) return VM_OK;
        if (drain_stream) {
            const hipError_t e = hipStreamSynchronize(drain_stream);
            if (e != hipSuccess) return vm_fail(VM_E_DEVICE, "hipStreamSynchronize before a reallocation: %s", hipGetErrorString(e));
        }
        reset();
        void *p = nullptr;
        const hipError_t e = K == VmMem::Device ? hipMalloc(&p, n * sizeof(T)) : hipHostMalloc(&p, n * sizeof(T), hipHostMallocDefault);
        if (e != hipSuccess)
            return vm_fail(VM_E_DEVICE, "%s of %zu bytes: %s", K == VmMem::Device ? "hipMalloc" : "hipHostMalloc", n * sizeof(T),
                           hipGetErrorString(e));
        p_ = (T *)p;
        n_ = n;
        return VM_OK;
    }
    void reset()
    {
        if (p_) (void)(K == VmMem::Device ? hipFree(p_) : hipHostFree(p_));
        p_ = nullptr;
        n_ = 0;
    }
    // gives the allocation up without freeing it (its device cannot be made current)
    T *release()
    {
        T *p = p_;
        p_ = nullptr;
        n_ = 0;
        return p;
    }

private:
    T *p_ = nullptr;
    size_t n_ = 0;
};

template <class T> using VmDev = VmBuf<T, VmMem::Device>;
template <class T> using VmPinned = VmBuf<T, VmMem::Pinned>;

// One HIP event.
class VmEvent {
public:
    VmEvent() = default;
    VmEvent(VmEvent &&o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    VmEvent(const VmEvent &) = delete;
    VmEvent &operator=(const VmEvent &) = delete;
    ~VmEvent()
    {
        if (e_) (void)hipEventDestroy(e_);
    }

    hipEvent_t get() const { return e_; }
    int create(unsigned flags = hipEventDefault)
    {
        const hipError_t e = hipEventCreateWithFlags(&e_, flags);
        if (e != hipSuccess) {
            e_ = nullptr;
            return vm_fail(VM_E_DEVICE, "hipEventCreateWithFlags: %s", hipGetErrorString(e));
        }
        return VM_OK;
    }

private:
    hipEvent_t e_ = nullptr;
};

#endif
