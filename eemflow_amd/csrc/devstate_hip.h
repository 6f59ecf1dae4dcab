// The HIP-facing halves of devstate.h (included at the end of common.h, which defines EEM_HIP_CHECK): the only place of csrc/ that sets a
// kernel's dynamic-LDS limit or reads the CU count, the scratch-arena pool, and the growing device buffer of the three contexts.
#pragma once
#include "devstate.h"

// Raises `kernel`'s dynamic-LDS limit on the current device to `bytes` unless `lim` says it is there already; in front of a launch
inline int eem_raise_lds(LdsLimit& lim, const void* kernel, int bytes) {
    int dev = 0;
    EEM_HIP_CHECK(hipGetDevice(&dev));
    return lim.raise(dev, bytes, [kernel](int b) {
        EEM_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, b));
        return EEM_OK;
    });
}
// the launch sites' form: one state object per site (and so per kernel instantiation); the kernel goes last because its template
// arguments may hold commas
#define EEM_RAISE_LDS(bytes, ...)                                                       \
    do {                                                                               \
        static LdsLimit _lim;                                                          \
        const int _rc = eem_raise_lds(_lim, (const void*)(__VA_ARGS__), (int)(bytes)); \
        if (_rc != EEM_OK) return _rc;                                                 \
    } while (0)

// CUs of the device, read once per process: the library runs on gfx950 only, every device of which a process sees is the same chip
inline int eem_cu_count() {
    static const int cus = [] {
        int d = 0, n = 256;
        hipDeviceProp_t p;
        if (hipGetDevice(&d) == hipSuccess && hipGetDeviceProperties(&p, d) == hipSuccess) n = p.multiProcessorCount;
        return n > 0 ? n : 256;
    }();
    return cus;
}

// a device buffer that only grows (the old contents are not kept)
struct DevBuf {
    float* p = nullptr;
    size_t cap = 0;                    // floats
};
inline int devbuf_ensure(DevBuf& b, size_t floats) {
    if (floats <= b.cap) return EEM_OK;
    if (b.p) EEM_HIP_CHECK(hipFree(b.p));
    b.p = nullptr;
    b.cap = 0;
    EEM_HIP_CHECK(hipMalloc(&b.p, floats * sizeof(float)));
    b.cap = floats;
    return EEM_OK;
}

// A pool of scratch arenas, grown on demand and owned by the library, not by the calling thread (a loader's worker threads come and
// go): one per (device, stream) for up to eight streams, so that work in flight on different streams does not wait for each other; a
// ninth stream takes over the least recently used arena after waiting for the kernels that last used it (arena_choose).  A caller holds
// `lock` from take() over its launches to done(), so a take-over always sees the event of the arena's last user.
struct Arena {
    struct Slot { void* p = nullptr; size_t cap = 0; int dev = -1; hipEvent_t done = nullptr; void* stream = nullptr; unsigned long used = 0; };
    Slot slots[kArenaSlots];
    unsigned long tick = 0;
    std::mutex lock;

    // EEM_OK and *scratch of at least `need` bytes on the current device; *token is for done()
    int take(size_t need, void* stream, char** scratch, void** token) {
        int dev = 0;
        EEM_HIP_CHECK(hipGetDevice(&dev));
        ArenaSlotState st[kArenaSlots];
        for (int i = 0; i < kArenaSlots; ++i) st[i] = {slots[i].p != nullptr, slots[i].dev, slots[i].stream, slots[i].used};
        const ArenaChoice ch = arena_choose(st, dev, stream);
        Slot* ar = &slots[ch.slot];
        if (ch.wait) EEM_HIP_CHECK(hipStreamWaitEvent((hipStream_t)stream, ar->done, 0));
        ar->stream = stream;
        ar->used = ++tick;
        if (ar->p == nullptr || ar->dev != dev || ar->cap < need) {
            if (ar->p) {                                                             // hipFree synchronises with work using it
                if (ar->dev != dev) EEM_HIP_CHECK(hipSetDevice(ar->dev));
                EEM_HIP_CHECK(hipFree(ar->p));
                if (ar->dev != dev) { EEM_HIP_CHECK(hipEventDestroy(ar->done)); ar->done = nullptr; EEM_HIP_CHECK(hipSetDevice(dev)); }
            }
            ar->p = nullptr;
            ar->cap = need + need / 4;
            EEM_HIP_CHECK(hipMalloc(&ar->p, ar->cap));
            if (!ar->done) EEM_HIP_CHECK(hipEventCreateWithFlags(&ar->done, hipEventDisableTiming));
            ar->dev = dev;
        }
        *scratch = (char*)ar->p;
        *token = ar;
        return EEM_OK;
    }
    // records the arena's event behind the launches
    int done(void* token, void* stream) {
        EEM_HIP_CHECK(hipEventRecord(static_cast<Slot*>(token)->done, (hipStream_t)stream));
        return EEM_OK;
    }
};
