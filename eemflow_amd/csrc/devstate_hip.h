// The HIP-facing halves of devstate.h (included at the end of common.h, which defines EEM_HIP_CHECK): the only place of csrc/ that sets a
// kernel's dynamic-LDS limit or reads the CU count or the device's architecture, the scratch-arena pool, the growing device buffer of
// the three contexts, the stage recorder's arena and copy, and the stream carry's error text.
#pragma once
#include <string.h>

#include "devstate.h"
#include "stagerec.h"

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

// What every *_create starts with: `device` exists, is made current and is a gfx950
inline int ctx_open_device(const char* fn, int device) {
    int ndev = 0;
    EEM_HIP_CHECK(hipGetDeviceCount(&ndev));
    EEM_REQUIRE(device >= 0 && device < ndev, "%s: device %d of %d", fn, device, ndev);
    EEM_HIP_CHECK(hipSetDevice(device));
    hipDeviceProp_t prop;
    EEM_HIP_CHECK(hipGetDeviceProperties(&prop, device));
    EEM_REQUIRE(strncmp(prop.gcnArchName, "gfx950", 6) == 0, "%s: this library is built for gfx950 (MI355X) only; device %d is %s", fn,
                device, prop.gcnArchName);
    return EEM_OK;
}

// A device buffer that only grows (the old contents are not kept).  It owns its memory: a context's buffers go with the context, on
// the device that is current then (the *_destroy make the context's device current before `delete`); a move leaves the source empty.
struct DevBuf {
    float* p = nullptr;
    size_t cap = 0;                    // floats
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            if (p) (void)hipFree(p);
            p = o.p; cap = o.cap;
            o.p = nullptr; o.cap = 0;
        }
        return *this;
    }
    ~DevBuf() { if (p) (void)hipFree(p); }
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

// The stage recorder (stagerec.h) with its arena.  A call site tests the context's "this call records" flag first and does nothing
// else when it is off; nothing here launches a kernel.
struct DevStageRecorder : StageRecorder {
    DevBuf buf;

    // the head of every call that may record: the last call's records go; a recording call gets an arena of `floats`
    int begin_call(bool records, size_t floats) {
        begin();
        return records ? devbuf_ensure(buf, floats) : EEM_OK;
    }
    // `src` is [n][src_ctotal][h * w] (0: ch), of which the channels [src_coff, src_coff + ch) are copied on `st`, the stream of the
    // launch that has just written them
    int stage(const char* name, const char* form, const float* src, int n, int ch, int h, int w, hipStream_t st, int src_ctotal = 0,
              int src_coff = 0) {
        return file(name, form, n, ch, h, w, buf.cap, [&](size_t off) {
            const size_t hw = (size_t)h * w;
            float* dst = buf.p + off;
            if (src_ctotal == 0 || src_ctotal == ch)
                EEM_HIP_CHECK(hipMemcpyAsync(dst, src, (size_t)n * ch * hw * 4, hipMemcpyDeviceToDevice, st));
            else
                EEM_HIP_CHECK(hipMemcpy2DAsync(dst, (size_t)ch * hw * 4, src + (size_t)src_coff * hw, (size_t)src_ctotal * hw * 4,
                                               (size_t)ch * hw * 4, n, hipMemcpyDeviceToDevice, st));
            return EEM_OK;
        });
    }
    bool rerun() const { return overflowed(buf.cap); }
    // *_get_stage's recorded names: the record's copy and dims, or NULL
    const float* lookup(const char* name, int dims[4]) const {
        const StageRec* r = find(name);
        if (!r) return nullptr;
        for (int i = 0; i < 4; ++i) dims[i] = r->dims[i];
        return buf.p + r->off;
    }
    // *_stage_list: list() into the caller's buffer (NULL: only *need, the bytes it takes)
    int list_into(const char* fn, char* out, size_t cap, size_t* need_bytes) const {
        const std::string s = list();
        *need_bytes = s.size() + 1;
        if (out == nullptr) return EEM_OK;
        EEM_REQUIRE(cap >= s.size() + 1, "%s: the list needs %zu bytes, the buffer holds %zu", fn, s.size() + 1, cap);
        memcpy(out, s.c_str(), s.size() + 1);
        return EEM_OK;
    }
};

// A stream call that may not continue the carried window: the entry point's error.  (The wrappers key on "<prefix>_stream_reset".)
inline int stream_carry_check(const StreamCarry& k, const char* fn, const char* prefix, int h, int w, const int pad[4], int cin,
                              unsigned long wver) {
    const StreamCarry::Check r = k.check(h, w, pad, cin, wver);
    EEM_REQUIRE(r != StreamCarry::kWeightsChanged, "%s: the weights changed since the carried window was encoded; call %s_stream_reset to "
                "start a new stream", fn, prefix);
    EEM_REQUIRE(r != StreamCarry::kShapeChanged, "%s: the carried window is %dx%d (pad %d %d %d %d), this call's %dx%d (pad %d %d %d %d); call "
                "%s_stream_reset to start a new stream", fn, k.h, k.w, k.pad[0], k.pad[1], k.pad[2], k.pad[3], h, w, pad[0], pad[1], pad[2],
                pad[3], prefix);
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
