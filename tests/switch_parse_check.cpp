// Stand-alone host program (tests/test_switches_host.py builds and runs it): the accessors of eemflow_amd/csrc/switch.h parse one switch
// of every kind as the inline expressions they replaced did.  The expected values below are those expressions' results, written out:
//   ON1      e && e[0] == '1'            NOT0    !(e && e[0] == '0')          PRESENT  getenv(..) != nullptr
//   INT      e ? atoi(e) : default       LONG    e ? atol(e) : default        FLOAT    e ? (float)atof(e) : default
// Prints every mismatch and exits 1, or prints OK.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "switch.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static void put(const char* name, const char* value) {
    if (value) setenv(name, value, 1);
    else unsetenv(name);
}

int main() {
    static const char* const kValues[5] = {nullptr, "0", "1", "2", ""};       // unset first

    const bool on1[5] = {false, false, true, false, false};
    const bool not0[5] = {true, false, true, true, true};
    const bool present[5] = {false, true, true, true, true};
    const int ints[5] = {2, 0, 1, 2, 0};                                       // EEM_ERAFT_WNC_UPD: default 2
    const long longs[5] = {30000, 0, 1, 2, 0};                                 // EEM_WNC_SMALL_MAXPX: default 30000
    const float floats[5] = {0.f, 0.f, 1.f, 2.f, 0.f};                         // EEM_SKIP_SPIN_US: default 0
    for (int i = 0; i < 5; ++i) {
        const char* v = kValues[i];
        put("EEM_S2R", v);             CHECK(sw_on<SW_EEM_S2R>() == on1[i]);
        put("EEM_FEWOUT_WIDE", v);     CHECK(sw_not0<SW_EEM_FEWOUT_WIDE>() == not0[i]);
        put("EEM_NO_ENC1", v);         CHECK(sw_present<SW_EEM_NO_ENC1>() == present[i]);
        put("EEM_DEC_WNC", v);
        const char* raw = sw_raw<SW_EEM_DEC_WNC>();
        CHECK(v ? (raw && strcmp(raw, v) == 0) : raw == nullptr);
        put("EEM_ERAFT_WNC_UPD", v);   CHECK(sw_int<SW_EEM_ERAFT_WNC_UPD>() == ints[i]);
        put("EEM_WNC_SMALL_MAXPX", v); CHECK(sw_long<SW_EEM_WNC_SMALL_MAXPX>() == longs[i]);
        put("EEM_SKIP_SPIN_US", v);    CHECK(sw_float<SW_EEM_SKIP_SPIN_US>() == floats[i]);
    }
    put("EEM_S2R", "10");              CHECK(sw_on<SW_EEM_S2R>());               // only the first character counts
    put("EEM_S2R", "on");              CHECK(!sw_on<SW_EEM_S2R>());
    put("EEM_FEWOUT_WIDE", "01");      CHECK(!sw_not0<SW_EEM_FEWOUT_WIDE>());
    put("EEM_ERAFT_WNC_UPD", "7x");    CHECK(sw_int<SW_EEM_ERAFT_WNC_UPD>() == 7);
    put("EEM_ERAFT_WNC_UPD", "-3");    CHECK(sw_int<SW_EEM_ERAFT_WNC_UPD>() == -3);
    put("EEM_WNC_SMALL_MAXPX", "4000000000"); CHECK(sw_long<SW_EEM_WNC_SMALL_MAXPX>() == 4000000000L);
    put("EEM_SKIP_SPIN_US", "1.5");    CHECK(sw_float<SW_EEM_SKIP_SPIN_US>() == 1.5f);

    // the other defaults that are no zero
    unsetenv("EEM_WINO");              CHECK(sw_int<SW_EEM_WINO>() == 1);
    unsetenv("EEM_COLWALK");           CHECK(sw_int<SW_EEM_COLWALK>() == ((1 << 6) | (1 << 7)));
    unsetenv("EEM_WALK3");             CHECK(sw_int<SW_EEM_WALK3>() == ((1 << 1) | (1 << 3) | (1 << 4) | (1 << 6) | (1 << 7)));
    unsetenv("EEM_PLUS_TAIL_MAXCIN");  CHECK(sw_int<SW_EEM_PLUS_TAIL_MAXCIN>() == 184);
    unsetenv("EEM_GCONVB_MINBLK");     CHECK(sw_long<SW_EEM_GCONVB_MINBLK>() == 64);
    unsetenv("EEM_SPLITK_MAX");        CHECK(sw_long<SW_EEM_SPLITK_MAX>() == 512);
    unsetenv("EEM_FEWOUT_SMALL_BLOCKS"); CHECK(sw_long<SW_EEM_FEWOUT_SMALL_BLOCKS>() == 512);
    unsetenv("EEM_SKIP_SPIN_BLOCKS");  CHECK(sw_int<SW_EEM_SKIP_SPIN_BLOCKS>() == 1);

    // families: the site completes the name; the bare prefix is a name of its own
    unsetenv("EEM_V16_32"); unsetenv("EEM_V32_64");
    CHECK(sw_family<SW_EEM_V>("16_32") == nullptr);
    put("EEM_V16_32", "103");
    CHECK(sw_family<SW_EEM_V>("16_32") && atoi(sw_family<SW_EEM_V>("16_32")) == 103);
    CHECK(sw_family<SW_EEM_V>("32_64") == nullptr);
    unsetenv("EEM_ENC_PER_XCD"); unsetenv("EEM_ENC_PER_XCD_E1");
    CHECK(sw_family<SW_EEM_ENC_PER_XCD>("_E1") == nullptr && sw_family<SW_EEM_ENC_PER_XCD>("") == nullptr);
    put("EEM_ENC_PER_XCD", "12");
    CHECK(sw_family<SW_EEM_ENC_PER_XCD>("_E1") == nullptr && atoi(sw_family<SW_EEM_ENC_PER_XCD>("")) == 12);
    put("EEM_ENC_PER_XCD_E1", "20");
    CHECK(atoi(sw_family<SW_EEM_ENC_PER_XCD>("_E1")) == 20 && atoi(sw_family<SW_EEM_ENC_PER_XCD>("")) == 12);

    // read now follows a later change; read once keeps what its first call saw
    put("EEM_WGRAD_LAST_SIDE", "1");   CHECK(sw_on_once<SW_EEM_WGRAD_LAST_SIDE>() && sw_on<SW_EEM_WGRAD_LAST_SIDE>());
    put("EEM_WGRAD_LAST_SIDE", "0");   CHECK(sw_on_once<SW_EEM_WGRAD_LAST_SIDE>() && !sw_on<SW_EEM_WGRAD_LAST_SIDE>());
    unsetenv("EEM_WGRAD_LAST_SIDE");   CHECK(sw_on_once<SW_EEM_WGRAD_LAST_SIDE>() && !sw_on<SW_EEM_WGRAD_LAST_SIDE>());
    put("EEM_WALK3_TRAIN", "0");       CHECK(!sw_not0_once<SW_EEM_WALK3_TRAIN>() && !sw_not0<SW_EEM_WALK3_TRAIN>());
    unsetenv("EEM_WALK3_TRAIN");       CHECK(!sw_not0_once<SW_EEM_WALK3_TRAIN>() && sw_not0<SW_EEM_WALK3_TRAIN>());
    unsetenv("EEM_COLWALK");           CHECK(sw_int_once<SW_EEM_COLWALK>() == 192);
    put("EEM_COLWALK", "5");           CHECK(sw_int_once<SW_EEM_COLWALK>() == 192 && sw_int<SW_EEM_COLWALK>() == 5);
    put("EEM_SPLITK_MAX", "64");       CHECK(sw_long_once<SW_EEM_SPLITK_MAX>() == 64);
    unsetenv("EEM_SPLITK_MAX");        CHECK(sw_long_once<SW_EEM_SPLITK_MAX>() == 64 && sw_long<SW_EEM_SPLITK_MAX>() == 512);
    put("EEM_SKIP_SPIN_US", "2.5");    CHECK(sw_float_once<SW_EEM_SKIP_SPIN_US>() == 2.5f);
    put("EEM_SKIP_SPIN_US", "4");      CHECK(sw_float_once<SW_EEM_SKIP_SPIN_US>() == 2.5f && sw_float<SW_EEM_SKIP_SPIN_US>() == 4.f);
    put("EEM_SKIP_KERNELS", "enc.");   CHECK(strcmp(sw_raw_once<SW_EEM_SKIP_KERNELS>(), "enc.") == 0);
    unsetenv("EEM_SKIP_KERNELS");      CHECK(sw_raw_once<SW_EEM_SKIP_KERNELS>() != nullptr && sw_raw<SW_EEM_SKIP_KERNELS>() == nullptr);

    if (failures == 0) printf("OK\n");
    return failures ? 1 : 0;
}
