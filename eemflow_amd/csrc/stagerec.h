// The stage recorder of the E-RAFT and EEMFlow+ contexts (the fp64 stage tests): which launch outputs are filed, where in the arena,
// and when a forward has to run again.  Plain C++, no HIP headers, like devstate.h: the device copy is handed in as a callable, so
// tests/stagerec_check.cpp runs every decision with no GPU.  devstate_hip.h holds the HIP-facing half (DevStageRecorder).
#pragma once
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

struct StageRec {                      // one recorded launch output: [dims] floats at the arena + off
    std::string name, form;
    int dims[4];
    size_t off;
};

// The copies live in one arena sized by the forward before (`need`): a forward whose records do not fit only measures them and is
// run again with the arena grown (overflowed).
struct StageRecorder {
    bool on = false;
    std::vector<std::string> prefix;
    std::vector<StageRec> rec;
    size_t used = 0, need = 0;         // floats: filed or measured by the call under way / the most a recording call has needed

    // comma-separated name prefixes; NULL = off; an empty prefix matches every name
    void set_prefixes(const char* list) {
        prefix.clear();
        on = list != nullptr;
        if (!on) return;
        const std::string all(list);
        for (size_t i = 0; i <= all.size();) {
            size_t j = all.find(',', i);
            if (j == std::string::npos) j = all.size();
            prefix.push_back(all.substr(i, j - i));
            i = j + 1;
        }
    }
    void begin() { rec.clear(); used = 0; }
    // Files [n][ch][h][w] under `name` if a prefix matches: copy(offset in floats) -> 0 or an error, which is returned.  A record
    // that does not fit into `arena_cap` floats is only measured - and so is every later one of the call, `used` never shrinks.
    template <class Copy>
    int file(const char* name, const char* form, int n, int ch, int h, int w, size_t arena_cap, Copy&& copy) {
        bool wanted = false;
        for (const std::string& p : prefix) wanted = wanted || strncmp(name, p.c_str(), p.size()) == 0;
        if (!wanted) return 0;
        const size_t cnt = (size_t)n * ch * h * w, off = used;
        used += (cnt + 63) & ~(size_t)63;
        if (used > arena_cap) return 0;
        const int rc = copy(off);
        if (rc != 0) return rc;
        rec.push_back(StageRec{name, form ? form : "", {n, ch, h, w}, off});
        return 0;
    }
    // the call just made only measured: the same call again, its arena grown to `need`, files every record
    bool overflowed(size_t arena_cap) const { return on && used > arena_cap; }
    void end() { need = need > used ? need : used; }       // (after a recording call)
    const StageRec* find(const char* name) const {
        for (const StageRec& r : rec)
            if (r.name == name) return &r;
        return nullptr;
    }
    // "name form|- n c h w\n" per record, in launch order
    std::string list() const {
        std::string s;
        for (const StageRec& r : rec) {
            char line[160];
            snprintf(line, sizeof(line), "%s %s %d %d %d %d\n", r.name.c_str(), r.form.empty() ? "-" : r.form.c_str(), r.dims[0], r.dims[1],
                     r.dims[2], r.dims[3]);
            s += line;
        }
        return s;
    }
};
