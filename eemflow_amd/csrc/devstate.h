// Host-side state the launchers keep per device, and the small host helpers the three C ABIs share.  Plain C++, no HIP headers: what a
// decision must call is handed in as a callable, so tests/devstate_check.cpp runs the decisions with no GPU.  devstate_hip.h holds the
// HIP-facing halves (eem_raise_lds, Arena, DevBuf, eem_cu_count).
#pragma once
#include <stddef.h>

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
