// Every environment switch of the native library is a row of switches.def.h; this header holds the only getenv calls of csrc/.
// One accessor per parse kind.  Each takes the switch as a template argument and checks at compile time that the row declares that
// kind, so the table cannot disagree with a site about how a switch is parsed.  sw_x<S>() reads the environment now (sites that run per
// call, at load, at schedule build or inside a site's own static); sw_x_once<S>() reads it at its first call in the process and is
// only for rows marked ONCE.
#pragma once
#include <stdio.h>
#include <stdlib.h>

enum SwKind { SW_ON1, SW_NOT0, SW_PRESENT, SW_RAW, SW_INT, SW_LONG, SW_FLOAT, SW_FAMILY };
enum SwWhen { SW_CALL, SW_ONCE, SW_LOAD, SW_BUILD };

enum Sw {
#define SW(name, kind, dflt, when, text) SW_##name,
#include "switches.def.h"
#undef SW
    SW_COUNT
};

struct SwRow { const char* name; SwKind kind; double dflt; SwWhen when; };
constexpr SwRow kSwitches[SW_COUNT + 1] = {
#define SW(name, kind, dflt, when, text) {#name, SW_##kind, dflt, SW_##when},
#include "switches.def.h"
#undef SW
    {nullptr, SW_RAW, 0, SW_CALL}};

template <Sw S, SwKind K>
inline const char* sw_env() {
    static_assert(kSwitches[S].kind == K, "switches.def.h declares another parse kind for this switch");
    return getenv(kSwitches[S].name);
}
template <Sw S> constexpr bool sw_is_once() { return kSwitches[S].when == SW_ONCE; }

// the value is '1...' / anything but '0...' / merely set / the string itself (tri-states, words, defaults computed at the site)
template <Sw S> inline bool sw_on() { const char* e = sw_env<S, SW_ON1>(); return e && e[0] == '1'; }
template <Sw S> inline bool sw_not0() { const char* e = sw_env<S, SW_NOT0>(); return !(e && e[0] == '0'); }
template <Sw S> inline bool sw_present() { return sw_env<S, SW_PRESENT>() != nullptr; }
template <Sw S> inline const char* sw_raw() { return sw_env<S, SW_RAW>(); }
// numbers: atoi / atol / atof of the value, the row's default when unset
template <Sw S> inline int sw_int() { const char* e = sw_env<S, SW_INT>(); return e ? atoi(e) : (int)kSwitches[S].dflt; }
template <Sw S> inline long sw_long() { const char* e = sw_env<S, SW_LONG>(); return e ? atol(e) : (long)kSwitches[S].dflt; }
template <Sw S> inline float sw_float() { const char* e = sw_env<S, SW_FLOAT>(); return e ? (float)atof(e) : (float)kSwitches[S].dflt; }
// (sw_raw_once keeps getenv's pointer: it stays valid while nothing sets that variable again)
// a family: the row's name is a prefix, the site supplies the rest; the bare prefix reads with suffix ""
template <Sw S> inline const char* sw_family(const char* suffix) {
    static_assert(kSwitches[S].kind == SW_FAMILY, "not a family row");
    char name[64];
    snprintf(name, sizeof name, "%s%s", kSwitches[S].name, suffix);
    return getenv(name);
}

typedef const char* SwStr;
#define SW_ONCE_FORM(type, fn) \
    template <Sw S> inline type fn##_once() { static_assert(sw_is_once<S>(), "row is not read once per process"); static const type v = fn<S>(); return v; }
SW_ONCE_FORM(bool, sw_on)
SW_ONCE_FORM(bool, sw_not0)
SW_ONCE_FORM(bool, sw_present)
SW_ONCE_FORM(SwStr, sw_raw)
SW_ONCE_FORM(int, sw_int)
SW_ONCE_FORM(long, sw_long)
SW_ONCE_FORM(float, sw_float)
#undef SW_ONCE_FORM
