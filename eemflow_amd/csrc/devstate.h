// Host-side state the launchers keep per device, and the small host helpers the three C ABIs share.  Plain C++, no HIP headers: what a
// decision must call is handed in as a callable, so tests/devstate_check.cpp runs the decisions with no GPU.  devstate_hip.h holds the
// HIP-facing halves (eem_raise_lds, Arena, DevBuf, eem_cu_count, ctx_open_device, stream_carry_check); stagerec.h the stage recorder.
#pragma once
#include <stddef.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <vector>

constexpr int kDevTable = 16;          // devices with a slot in a per-device table; an index outside it is served without the table

// ------------------------------------------------------------------------------- per-device dynamic-LDS limit of one kernel
// A kernel's limit is an attribute per DEVICE, and a context sets its device per call: one `static LdsLimit` per kernel instantiation
// remembers the bytes each device was raised to.  raise() is one atomic load once a device has its limit; a launch that needs more
// takes the lock, and only a successful set(bytes) (0 = success, else the error raise() returns) is recorded.
struct LdsLimit {
    std::atomic<int> mark[kDevTable] = {};
    std::mutex lock;

    template <class Set>
    int raise(int dev, int bytes, Set&& set) {
        if (dev < 0 || dev >= kDevTable) return set(bytes);
        if (bytes <= mark[dev].load(std::memory_order_acquire)) return 0;
        std::lock_guard<std::mutex> guard(lock);
        if (bytes <= mark[dev].load(std::memory_order_relaxed)) return 0;
        const int rc = set(bytes);
        if (rc == 0) mark[dev].store(bytes, std::memory_order_release);
        return rc;
    }
};

// ------------------------------------------------------------------------------- scratch-arena slots
// Which of a pool's slots serves (dev, stream): the slot that already does; else an empty one; else the least recently used, and the
// caller's stream must first wait for that slot's last user when the slot lives on the same device (another device's memory is freed,
// which synchronises).
constexpr int kArenaSlots = 8;
struct ArenaSlotState { bool in_use; int dev; const void* stream; unsigned long tick; };
struct ArenaChoice { int slot; bool wait; };

inline ArenaChoice arena_choose(const ArenaSlotState (&s)[kArenaSlots], int dev, const void* stream) {
    for (int i = 0; i < kArenaSlots; ++i)
        if (s[i].in_use && s[i].dev == dev && s[i].stream == stream) return {i, false};
    int k = 0;
    for (int i = 1; i < kArenaSlots; ++i)
        if ((!s[i].in_use && s[k].in_use) || (s[i].in_use == s[k].in_use && s[i].tick < s[k].tick)) k = i;
    return {k, s[k].in_use && s[k].dev == dev};
}

// ------------------------------------------------------------------------------- weights: reading a flat state_dict, packing an arena
struct Cursor {
    const float* p;
    const float* end;
    const float* take(size_t n) { const float* r = p; p += n; return r; }
};

struct Packer {                        // every piece starts on a multiple of 4 floats (16-byte loads); the padding is zeros
    std::vector<float> host;
    size_t push(size_t n) { size_t off = host.size(); host.resize(off + ((n + 3) & ~(size_t)3), 0.f); return off; }
};

// ------------------------------------------------------------------------------- the window a stream call carries to the next
// What the three *_forward_stream entry points remember of the last window they encoded (the window itself - feature maps, padded
// volume, flow - stays with the model).  A call checks the record, clears it BEFORE it launches anything, so that a failed call leaves
// no carry behind, and takes its own values after success.
struct StreamCarry {
    enum Check { kOk, kWeightsChanged, kShapeChanged };
    bool on = false;
    int h = 0, w = 0, pad[4] = {0, 0, 0, 0}, cin = 0;
    unsigned long wver = 0;            // the context's weights version the window was encoded with

    // may a call with these values continue the carried window?  (no carry: any call may start one)
    Check check(int h_, int w_, const int pad_[4], int cin_, unsigned long wver_) const {
        if (!on) return kOk;
        if (wver != wver_ || cin != cin_) return kWeightsChanged;
        if (h != h_ || w != w_ || memcmp(pad, pad_, sizeof(pad)) != 0) return kShapeChanged;
        return kOk;
    }
    int pairs(int nvol) const { return on ? nvol : nvol - 1; }   // consecutive pairs that nvol new windows make
    void clear() { on = false; }
    void take(int h_, int w_, const int pad_[4], int cin_, unsigned long wver_) {
        on = true;
        h = h_; w = w_; cin = cin_; wver = wver_;
        memcpy(pad, pad_, sizeof(pad));
    }
};

// ------------------------------------------------------------------------------- the 9x9 correlation's 53 taps (EEMFlow, EEMFlow+)
inline constexpr int kTaps53[53] = {0,  2,  4,  6,  8,  10, 12, 14, 16, 18, 20, 21, 22, 23, 24, 26, 28, 29,
                                    30, 31, 32, 33, 34, 36, 38, 39, 40, 41, 42, 44, 46, 47, 48, 49, 50, 51,
                                    52, 54, 56, 57, 58, 59, 60, 62, 64, 66, 68, 70, 72, 74, 76, 78, 80};
