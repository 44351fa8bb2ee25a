// vm_rccl.cpp -- the RCCL side of the C-ABI: the broadcast of the shared parameter block (and of
// any byte payload) from one context to the others, for multi-GPU drivers.
#include "vm_host.h"

#include <dlfcn.h>
#include <mutex>
#include <vector>

// RCCL is resolved at first use so that the library loads (and the CPU-side
// tests run) on hosts without a usable librccl.
namespace {
struct Rccl {
    typedef int (*bcast_fn)(const void *, void *, size_t, int, int, void *, hipStream_t);
    typedef int (*initall_fn)(void **, int, const int *);
    typedef int (*destroy_fn)(void *);
    typedef int (*group_fn)(void);
    bcast_fn bcast = nullptr;
    initall_fn init_all = nullptr;
    destroy_fn destroy = nullptr;
    group_fn group_start = nullptr, group_end = nullptr;
    bool tried = false;
};
Rccl &rccl()
{
    static Rccl r;
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    if (!r.tried) {
        r.tried = true;
        // an RCCL the process already holds first (a host framework's own copy: RCCL and the HIP runtime must come
        // from ONE ROCm installation), then the system's
        void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL | RTLD_NOLOAD);
        if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL | RTLD_NOLOAD);
        if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (h) {
            r.bcast = (Rccl::bcast_fn)dlsym(h, "ncclBroadcast");
            r.init_all = (Rccl::initall_fn)dlsym(h, "ncclCommInitAll");
            r.destroy = (Rccl::destroy_fn)dlsym(h, "ncclCommDestroy");
            r.group_start = (Rccl::group_fn)dlsym(h, "ncclGroupStart");
            r.group_end = (Rccl::group_fn)dlsym(h, "ncclGroupEnd");
        }
    }
    return r;
}
const int kNcclInt8 = 0; // ncclDataType_t: ncclInt8 / ncclChar
} // namespace

extern "C" int vm_rccl_bcast(vm_ctx *c, void *comm, void *dev_buf, uint64_t bytes, int root)
{
    if (!c || !comm || !dev_buf) return vm_fail(VM_E_INVALID, "vm_rccl_bcast: NULL argument");
    VM_ON_DEVICE(c);
    Rccl &R = rccl();
    if (!R.bcast) return vm_fail(VM_E_DEVICE, "vm_rccl_bcast: cannot load librccl / ncclBroadcast");
    int rc = R.bcast(dev_buf, dev_buf, (size_t)bytes, kNcclInt8, root, comm, c->stream);
    if (rc != 0) return vm_fail(VM_E_DEVICE, "vm_rccl_bcast: ncclBroadcast returned %d", rc);
    return VM_OK;
}

// ncclCommInitAll: one communicator per device of ONE process (the C++ multi-device driver, examples/solve_shard.cpp)
extern "C" int vm_rccl_comm_init_all(int n, const int *devices, void **comms_out)
{
    if (n < 1 || !devices || !comms_out) return vm_fail(VM_E_INVALID, "vm_rccl_comm_init_all: bad argument");
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j)
            if (devices[i] == devices[j])
                return vm_fail(VM_E_INVALID, "vm_rccl_comm_init_all: device %d listed twice (RCCL wants one rank per device; contexts "
                                             "that share a device pass comms = NULL to vm_bcast_params)", devices[i]);
    Rccl &R = rccl();
    if (!R.init_all) return vm_fail(VM_E_DEVICE, "vm_rccl_comm_init_all: cannot load librccl / ncclCommInitAll");
    (void)hipGetLastError();
    int rc = R.init_all(comms_out, n, devices);
    (void)hipGetLastError();           // RCCL leaves stale errors behind when it probes peers
    if (rc != 0) return vm_fail(VM_E_DEVICE, "vm_rccl_comm_init_all: ncclCommInitAll returned %d", rc);
    return VM_OK;
}

extern "C" void vm_rccl_comm_destroy(void *comm)
{
    Rccl &R = rccl();
    if (comm && R.destroy) R.destroy(comm);
}

// One process, n contexts: a byte payload goes root -> every context (SURVEY 8(e)'s "exactly one ncclBroadcast of the
// shared parameter block"; for config[4] the block is followed by the frames' point constraints, so the payload's length
// is the caller's).
//   comms != NULL: comms[i] = the ncclComm_t of ctxs[i] (vm_rccl_comm_init_all); the payload is staged in a device
//                  buffer per context and broadcast inside one ncclGroup over xGMI, each on its context's stream;
//   comms == NULL: TEST MODE for contexts that share a device (RCCL refuses two ranks on one device): the root's
//                  device buffer is copied device-to-device into the others'.
// Every context then reads ITS device copy back into dst_host[i] (bytes each): what travelled, not what was sent.
extern "C" int vm_bcast_bytes(vm_ctx *const *ctxs, void *const *comms, int n, int root, const void *src, uint64_t bytes,
                              void *const *dst_host)
{
    if (!ctxs || n < 1 || root < 0 || root >= n || !src || bytes == 0 || !dst_host) return vm_fail(VM_E_INVALID, "vm_bcast_bytes: bad argument");
    for (int i = 0; i < n; ++i)
        if (!ctxs[i] || !dst_host[i] || (comms && !comms[i])) return vm_fail(VM_E_INVALID, "vm_bcast_bytes: context / buffer / communicator %d is NULL", i);
    Rccl &R = rccl();
    if (comms && (!R.bcast || !R.group_start || !R.group_end)) return vm_fail(VM_E_DEVICE, "vm_bcast_bytes: cannot load librccl");
    std::vector<VmDev<char>> buf(n);
    int rc = VM_OK;
    auto fail = [&](int code, const char *what) { rc = vm_fail(code, "vm_bcast_bytes: %s", what); };
    for (int i = 0; i < n && rc == VM_OK; ++i) {
        VmDeviceGuard g(ctxs[i]->device);
        if (!g.ok || buf[i].reserve((size_t)bytes) != VM_OK) { fail(VM_E_DEVICE, "device buffer"); break; }
        // everybody but the root starts from zeros: what it ends up with is what travelled
        hipError_t e = i == root ? hipMemcpyAsync(buf[i].get(), src, (size_t)bytes, hipMemcpyHostToDevice, ctxs[i]->stream)
                                 : hipMemsetAsync(buf[i].get(), 0, (size_t)bytes, ctxs[i]->stream);
        if (e == hipSuccess && i == root) e = hipStreamSynchronize(ctxs[i]->stream);      // src belongs to the caller
        if (e != hipSuccess) fail(VM_E_DEVICE, hipGetErrorString(e));
    }
    if (rc == VM_OK && comms) {
        if (R.group_start() != 0) fail(VM_E_DEVICE, "ncclGroupStart");
        for (int i = 0; i < n && rc == VM_OK; ++i) {
            VmDeviceGuard g(ctxs[i]->device);
            if (!g.ok || R.bcast(buf[i].get(), buf[i].get(), (size_t)bytes, kNcclInt8, root, comms[i], ctxs[i]->stream) != 0)
                fail(VM_E_DEVICE, "ncclBroadcast");
        }
        if (R.group_end() != 0 && rc == VM_OK) fail(VM_E_DEVICE, "ncclGroupEnd");
    } else if (rc == VM_OK) {
        VmDeviceGuard g(ctxs[root]->device);
        if (hipStreamSynchronize(ctxs[root]->stream) != hipSuccess) fail(VM_E_DEVICE, "sync");
        for (int i = 0; i < n && rc == VM_OK; ++i)
            if (i != root && hipMemcpyAsync(buf[i].get(), buf[root].get(), (size_t)bytes, hipMemcpyDeviceToDevice, ctxs[i]->stream) != hipSuccess)
                fail(VM_E_DEVICE, "device-to-device copy");
    }
    for (int i = 0; i < n && rc == VM_OK; ++i) {
        VmDeviceGuard g(ctxs[i]->device);
        if (hipMemcpyAsync(dst_host[i], buf[i].get(), (size_t)bytes, hipMemcpyDeviceToHost, ctxs[i]->stream) != hipSuccess ||
            hipStreamSynchronize(ctxs[i]->stream) != hipSuccess) { fail(VM_E_DEVICE, "read-back"); break; }
    }
    for (int i = 0; i < n; ++i) { // each buffer is freed on its own device
        VmDeviceGuard g(ctxs[i]->device);
        if (g.ok) buf[i].reset();
        else buf[i].release();
    }
    (void)hipGetLastError();
    return rc;
}

// The shared parameter block root -> every context (vm_bcast_bytes), and each context adopts what IT received: kernel
// parameters + arithmetic mode.  blocks_out (n entries, may be NULL) receives the block as each context got it.
extern "C" int vm_bcast_params(vm_ctx *const *ctxs, void *const *comms, int n, int root, const vm_param_block *blk,
                               vm_param_block *blocks_out)
{
    if (!ctxs || n < 1 || root < 0 || root >= n || !blk) return vm_fail(VM_E_INVALID, "vm_bcast_params: bad argument");
    std::vector<vm_param_block> got(n);
    std::vector<void *> dst(n);
    for (int i = 0; i < n; ++i) dst[i] = &got[i];
    int rc = vm_bcast_bytes(ctxs, comms, n, root, blk, sizeof(vm_param_block), dst.data());
    for (int i = 0; i < n && rc == VM_OK; ++i) {
        if ((rc = vm_set_params(ctxs[i], &got[i].kp)) != VM_OK) break;
        if ((rc = vm_set_math_mode(ctxs[i], got[i].math_mode)) != VM_OK) break;
        if (blocks_out) blocks_out[i] = got[i];
    }
    return rc;
}
