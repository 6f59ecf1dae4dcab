// Stand-alone host program (tests/test_devstate_host.py builds and runs it): the decisions of eemflow_amd/csrc/devstate.h with a counting
// fake in place of the HIP call - when a kernel's dynamic-LDS limit is set again (per device, per size, after a failure, from eight
// threads at once) and which scratch-arena slot serves a (device, stream).  Prints every mismatch and exits 1, or prints OK.
#include <stdio.h>

#include <thread>

#include "devstate.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static void check_lds_limit() {
    LdsLimit lim;
    int sets = 0, last = 0, fail_with = 0;
    auto set = [&](int bytes) { ++sets; last = bytes; return fail_with; };

    CHECK(lim.raise(0, 96 * 1024, set) == 0 && sets == 1 && last == 96 * 1024);      // the first call on device 0 sets
    CHECK(lim.raise(0, 96 * 1024, set) == 0 && sets == 1);                           // the same bytes again: nothing
    CHECK(lim.raise(1, 96 * 1024, set) == 0 && sets == 2);                           // device 1 has its own limit
    CHECK(lim.raise(1, 96 * 1024, set) == 0 && sets == 2);
    CHECK(lim.raise(0, 128 * 1024, set) == 0 && sets == 3 && last == 128 * 1024);    // more: set again
    CHECK(lim.raise(0, 64 * 1024, set) == 0 && sets == 3);                           // less: nothing
    CHECK(lim.raise(1, 128 * 1024, set) == 0 && sets == 4);                          // (device 1 was still at 96 KB)

    fail_with = 2;                                                                   // a failed set records nothing
    CHECK(lim.raise(2, 96 * 1024, set) == 2 && sets == 5);
    CHECK(lim.raise(2, 96 * 1024, set) == 2 && sets == 6);
    fail_with = 0;
    CHECK(lim.raise(2, 96 * 1024, set) == 0 && sets == 7);                           // the next call tries again
    CHECK(lim.raise(2, 96 * 1024, set) == 0 && sets == 7);
    fail_with = 2;
    CHECK(lim.raise(0, 160 * 1024, set) == 2 && sets == 8);                          // ... and a failure keeps the old mark
    fail_with = 0;
    CHECK(lim.raise(0, 128 * 1024, set) == 0 && sets == 8);
    CHECK(lim.raise(0, 160 * 1024, set) == 0 && sets == 9);

    for (int i = 0; i < 3; ++i) {                                                    // outside the table: every call sets
        CHECK(lim.raise(kDevTable, 96 * 1024, set) == 0 && sets == 10 + 2 * i);
        CHECK(lim.raise(-1, 96 * 1024, set) == 0 && sets == 11 + 2 * i);
    }
    CHECK(lim.raise(kDevTable - 1, 96 * 1024, set) == 0 && lim.raise(kDevTable - 1, 96 * 1024, set) == 0 && sets == 16);
    static_assert(kDevTable == 16, "the table serves 16 devices");

    // eight threads, one state, one size, one device: exactly one set
    LdsLimit shared;
    std::atomic<int> nsets{0}, errors{0};
    std::atomic<bool> go{false};
    std::thread th[8];
    for (std::thread& t : th)
        t = std::thread([&] {
            while (!go.load()) {}
            for (int i = 0; i < 1000; ++i)
                if (shared.raise(3, 160 * 1024, [&](int) { ++nsets; return 0; }) != 0) ++errors;
        });
    go.store(true);
    for (std::thread& t : th) t.join();
    CHECK(nsets.load() == 1 && errors.load() == 0);
}

static void check_arena_choose() {
    int streams[12] = {};                                                               // addresses that stand for streams
    ArenaSlotState s[kArenaSlots] = {};
    for (int i = 0; i < kArenaSlots; ++i) s[i] = {false, -1, nullptr, 0};
    static_assert(kArenaSlots == 8, "eight slots");

    ArenaChoice c = arena_choose(s, 0, &streams[0]);
    CHECK(c.slot == 0 && !c.wait);                                                   // all empty: the first, no wait
    s[0] = {true, 0, &streams[0], 1};
    s[1] = {true, 0, &streams[1], 2};
    s[5] = {true, 0, &streams[5], 3};
    c = arena_choose(s, 0, &streams[1]);
    CHECK(c.slot == 1 && !c.wait);                                                   // its own slot again
    c = arena_choose(s, 0, &streams[5]);
    CHECK(c.slot == 5 && !c.wait);
    c = arena_choose(s, 0, &streams[9]);
    CHECK(c.slot == 2 && !c.wait);                                                   // an empty slot before any used one, however old
    c = arena_choose(s, 1, &streams[1]);
    CHECK(c.slot == 2 && !c.wait);                                                   // the same stream on another device does not match
    c = arena_choose(s, 0, nullptr);
    CHECK(c.slot == 2 && !c.wait);                                                   // (the NULL stream is a stream like any other)

    const unsigned long ticks[kArenaSlots] = {14, 12, 19, 11, 17, 13, 18, 16};       // all in use: the least recently used
    for (int i = 0; i < kArenaSlots; ++i) s[i] = {true, i == 3 ? 1 : 0, &streams[i], ticks[i]};
    c = arena_choose(s, 0, &streams[9]);
    CHECK(c.slot == 3 && !c.wait);                                                   // ... on another device: freed, not waited for
    c = arena_choose(s, 1, &streams[9]);
    CHECK(c.slot == 3 && c.wait);                                                    // ... on the caller's device: wait for its last user
    c = arena_choose(s, 1, &streams[3]);
    CHECK(c.slot == 3 && !c.wait);                                                   // (its own slot needs no wait)
    s[3].tick = 20;
    c = arena_choose(s, 0, &streams[9]);
    CHECK(c.slot == 1 && c.wait);                                                    // the next oldest, same device
    c = arena_choose(s, 0, &streams[3]);
    CHECK(c.slot == 1 && c.wait);                                                    // stream 3 serves device 1 only: no match on device 0
    for (int i = 0; i < kArenaSlots; ++i) {                                          // every slot in turn can be the oldest
        for (int k = 0; k < kArenaSlots; ++k) s[k] = {true, 0, &streams[k], 100ul + k};
        s[i].tick = 50;
        c = arena_choose(s, 0, &streams[10]);
        CHECK(c.slot == i && c.wait);
    }
}

int main() {
    check_lds_limit();
    check_arena_choose();
    if (failures == 0) printf("OK\n");
    return failures ? 1 : 0;
}
