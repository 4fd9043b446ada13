// rn_lds_grant (common.hpp): the one place that raises a kernel's dynamic-LDS limit above the 64 KiB default.
// The attribute belongs to the function ON THE CURRENT DEVICE, so it is raised per (kernel, device): a process that drives a second GPU must
// raise it there too.  Per pair the table keeps the largest size granted and the smallest refused (two call sites use the call as the query
// "does this much fit a workgroup of this device?" and fall back when it does not); the runtime is asked only for a size between the two.
// A launch path reads `granted` with one atomic load; everything else runs under one mutex, so concurrent host threads can neither skip a
// raise nor lower a limit another thread has just raised.  A device index or a kernel the table has no room for is asked every time.
#include "common.hpp"
#include <atomic>
#include <mutex>

#define LG_KERNELS 128                          // open-addressed by kernel address; the library has about 40 kernels above 64 KiB
#define LG_DEVS 32

struct LgSlot {
    std::atomic<const void*> kernel;
    std::atomic<unsigned> granted[LG_DEVS];     // bytes; 0 = nothing yet
    unsigned refused[LG_DEVS];                  // bytes; 0 = nothing yet (under the mutex)
    hipError_t refused_rc[LG_DEVS];
};
static LgSlot g_lg[LG_KERNELS];
static std::mutex g_lg_mutex;

// insert: under the mutex only
static LgSlot* lg_find(const void* kernel, bool insert) {
    const unsigned h = (unsigned)(((uintptr_t)kernel >> 4) * 0x9E3779B97F4A7C15ull >> 56);
    for (unsigned i = 0; i < LG_KERNELS; ++i) {
        LgSlot* s = &g_lg[(h + i) & (LG_KERNELS - 1)];
        const void* k = s->kernel.load(std::memory_order_acquire);
        if (k == kernel) return s;
        if (!k) {
            if (insert) s->kernel.store(kernel, std::memory_order_release);
            return insert ? s : nullptr;
        }
    }
    return nullptr;
}

hipError_t rn_lds_grant(const void* kernel, size_t bytes) {
    if (bytes <= 64 * 1024) return hipSuccess;
    int dev = -1;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const bool slotted = dev >= 0 && dev < LG_DEVS;
    LgSlot* s = slotted ? lg_find(kernel, false) : nullptr;
    if (s && bytes <= s->granted[dev].load(std::memory_order_acquire)) return hipSuccess;
    std::lock_guard<std::mutex> lock(g_lg_mutex);
    if (slotted && !s) s = lg_find(kernel, true);
    if (s) {
        if (bytes <= s->granted[dev].load(std::memory_order_relaxed)) return hipSuccess;
        if (s->refused[dev] && bytes >= s->refused[dev]) return s->refused_rc[dev];
    }
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (s) { s->refused[dev] = (unsigned)bytes; s->refused_rc[dev] = e; }
        return e;
    }
    if (s) s->granted[dev].store((unsigned)bytes, std::memory_order_release);
    return hipSuccess;
}
