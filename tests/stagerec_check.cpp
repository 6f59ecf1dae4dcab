// Stand-alone host program (tests/test_devstate_host.py builds and runs it): the decisions of eemflow_amd/csrc/stagerec.h - which launch
// outputs the stage recorder files, where, and when a forward runs again - with a counting fake in place of the device copy, and of
// devstate.h's StreamCarry - when a stream call may continue the carried window.  Prints every mismatch and exits 1, or prints OK.
#include <stdio.h>

#include "devstate.h"
#include "stagerec.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static void check_prefixes() {
    StageRecorder r;
    CHECK(!r.on && r.prefix.empty());
    r.set_prefixes("a,b");
    CHECK(r.on && r.prefix.size() == 2 && r.prefix[0] == "a" && r.prefix[1] == "b");
    r.set_prefixes("");
    CHECK(r.on && r.prefix.size() == 1 && r.prefix[0].empty());             // one empty prefix ...
    int copies = 0;
    auto copy = [&](size_t) { ++copies; return 0; };
    r.begin();
    CHECK(r.file("anything", "f", 1, 1, 1, 1, 1000, copy) == 0 && copies == 1 && r.rec.size() == 1);   // ... matches every name
    r.set_prefixes("it0.,,x");
    CHECK(r.prefix.size() == 3 && r.prefix[1].empty());
    r.set_prefixes(nullptr);
    CHECK(!r.on && r.prefix.empty());
    CHECK(r.rec.size() == 1);                                               // (switching off leaves the records to the caller)
    r.begin();
    CHECK(r.file("anything", "f", 1, 1, 1, 1, 1000, copy) == 0 && copies == 1 && r.rec.empty());        // no prefix: nothing matches
    CHECK(!r.overflowed(0));

    r.set_prefixes("fnet.,it0.");
    r.begin();
    CHECK(r.file("fnet.conv1", "", 1, 1, 1, 1, 1000, copy) == 0 && r.file("it0.corr", "", 1, 1, 1, 1, 1000, copy) == 0);
    CHECK(r.file("cnet.conv1", "", 1, 1, 1, 1, 1000, copy) == 0 && r.file("it1.corr", "", 1, 1, 1, 1, 1000, copy) == 0);
    CHECK(r.file("fnet", "", 1, 1, 1, 1, 1000, copy) == 0);                 // shorter than the prefix
    CHECK(copies == 3 && r.rec.size() == 2 && r.used == 128);               // a name that matches no prefix files and measures nothing
}

struct Call { const char* name; const char* form; int n, ch, h, w; };
static const Call kCalls[] = {{"pad", "pad", 2, 5, 7, 9},   {"enc0", nullptr, 2, 16, 4, 5}, {"skip", "x", 9, 9, 9, 9},
                              {"enc1", "wnc", 1, 64, 1, 1}, {"enc0", "second", 1, 1, 1, 3}, {"pred", "", 1, 2, 8, 8}};

// one pass over kCalls with an arena of `cap` floats; the offsets the copies were made at go to offs
static int run_pass(StageRecorder& r, size_t cap, std::vector<size_t>& offs) {
    int copies = 0;
    r.begin();
    for (const Call& c : kCalls)
        CHECK(r.file(c.name, c.form, c.n, c.ch, c.h, c.w, cap, [&](size_t off) { ++copies; offs.push_back(off); return 0; }) == 0);
    return copies;
}

static void check_arena() {
    StageRecorder r;
    r.set_prefixes("p,enc");
    std::vector<size_t> offs;
    // floats, each rounded up to 64: pad 630 -> 640, enc0 640, enc1 64, enc0 3 -> 64, pred 128: 1536
    CHECK(run_pass(r, 0, offs) == 0 && r.rec.empty() && r.used == 1536);    // need == 0: the first pass only measures
    CHECK(r.overflowed(0) && r.need == 0);
    r.end();
    CHECK(r.need == 1536);

    // an arena that holds the first two records: the third advances `used`, calls no copy and files nothing - nor does any later one,
    // even one that would fit into what is left
    offs.clear();
    CHECK(run_pass(r, 1280 + 32, offs) == 2 && r.rec.size() == 2 && r.used == 1536 && r.overflowed(1280 + 32));
    CHECK(offs.size() == 2 && offs[0] == 0 && offs[1] == 640);
    r.end();
    CHECK(r.need == 1536);

    // an arena of `need` floats: every record, at the same offsets in every pass
    offs.clear();
    CHECK(run_pass(r, r.need, offs) == 5 && r.rec.size() == 5 && !r.overflowed(r.need));
    const size_t want[5] = {0, 640, 1280, 1344, 1408};
    for (int i = 0; i < 5; ++i) CHECK(offs[i] == want[i] && r.rec[i].off == want[i] && want[i] % 64 == 0);
    std::vector<size_t> again;
    CHECK(run_pass(r, r.need + 100, again) == 5 && again == offs);
    CHECK(r.rec[1].name == "enc0" && r.rec[1].form.empty() && r.rec[1].dims[0] == 2 && r.rec[1].dims[1] == 16 && r.rec[1].dims[2] == 4 &&
          r.rec[1].dims[3] == 5);

    // find: the first of two equal names; list: "-" for an empty form
    const StageRec* hit = r.find("enc0");
    CHECK(hit == &r.rec[1] && hit->off == 640);
    CHECK(r.find("skip") == nullptr && r.find("enc") == nullptr);
    CHECK(r.list() == "pad pad 2 5 7 9\nenc0 - 2 16 4 5\nenc1 wnc 1 64 1 1\nenc0 second 1 1 1 3\npred - 1 2 8 8\n");

    // need never shrinks: a smaller call after a larger one
    r.begin();
    CHECK(r.file("p", "", 1, 1, 1, 1, r.need, [](size_t) { return 0; }) == 0 && r.used == 64);
    r.end();
    CHECK(r.need == 1536);
    r.begin();
    CHECK(r.file("p", "", 1, 1, 1, 2000, 4096, [](size_t) { return 0; }) == 0);
    r.end();
    CHECK(r.need == 2048);
    r.begin();
    CHECK(r.rec.empty() && r.used == 0 && r.need == 2048 && r.list().empty());

    // a failing copy: its error is returned and nothing is filed
    CHECK(r.file("p", "", 1, 1, 1, 1, 4096, [](size_t) { return 2; }) == 2 && r.rec.empty());
    // the recorder off never asks for another run
    r.set_prefixes(nullptr);
    CHECK(!r.overflowed(0));
}

static void check_carry() {
    StreamCarry k;
    const int pad[4] = {1, 2, 3, 4};
    CHECK(!k.on && k.pairs(3) == 2 && k.pairs(1) == 0);                     // no carry: nvol - 1 pairs
    CHECK(k.check(64, 64, pad, 5, 7) == StreamCarry::kOk);                  // ... and any call may start a stream
    k.take(64, 96, pad, 5, 7);
    CHECK(k.on && k.pairs(3) == 3 && k.pairs(1) == 1);                      // a carry: nvol pairs
    CHECK(k.check(64, 96, pad, 5, 7) == StreamCarry::kOk);
    CHECK(k.check(64, 96, pad, 5, 8) == StreamCarry::kWeightsChanged);
    CHECK(k.check(64, 96, pad, 15, 7) == StreamCarry::kWeightsChanged);     // cin: other weights
    CHECK(k.check(32, 96, pad, 5, 7) == StreamCarry::kShapeChanged);
    CHECK(k.check(64, 64, pad, 5, 7) == StreamCarry::kShapeChanged);
    for (int i = 0; i < 4; ++i) {                                           // any single pad entry
        int p2[4] = {1, 2, 3, 4};
        p2[i] += 1;
        CHECK(k.check(64, 96, p2, 5, 7) == StreamCarry::kShapeChanged);
    }
    const int other[4] = {0, 0, 0, 0};
    CHECK(k.check(32, 32, other, 5, 8) == StreamCarry::kWeightsChanged);    // weights are reported before the shape

    // the protocol of a call: check, clear, run, take on success - a failed call leaves no carry
    auto call = [&](bool succeeds, int h, unsigned long wver) {
        if (k.check(h, 96, pad, 5, wver) != StreamCarry::kOk) return false;
        k.clear();
        if (!succeeds) return false;
        k.take(h, 96, pad, 5, wver);
        return true;
    };
    CHECK(call(true, 64, 7) && k.on);
    CHECK(!call(false, 64, 7) && !k.on && k.pairs(2) == 1);
    CHECK(call(true, 32, 9) && k.on && k.h == 32 && k.wver == 9);           // (the next call starts a new stream, of any shape)
    CHECK(!call(true, 64, 9) && k.on);                                      // a refused call leaves the carry as it was
    k.clear();
    CHECK(!k.on);
}

int main() {
    check_prefixes();
    check_arena();
    check_carry();
    if (failures) return 1;
    printf("OK\n");
    return 0;
}
