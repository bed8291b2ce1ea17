// Environment switches (M2M_*): the ONLY file of the library that calls getenv.
// getenv is not safe against a concurrent setenv, and a switch that is read again can flip a kernel form in the middle of a run,
// so no launch reads the environment: every switch is latched once into the handle it steers (SessionSwitches of m2m_session,
// with its EncSwitches; TrainSwitches of m2m_trainer, the plan of a frontend call), into one small struct at the top of a decode call, or,
// where there is no handle, into one process-wide static.  DESIGN.md lists every switch with its values, default and latch time;
// tests/test_switch_inventory_cpu.py keeps that table equal to the names passed to the helpers below.
#pragma once

#include <stdlib.h>

namespace m2m {
inline const char* env_str(const char* name) { return getenv(name); }                  // the value, or null when unset
inline bool env_set(const char* name) { return getenv(name) != nullptr; }                // set at all, to any value
inline bool env_on(const char* name) { const char* v = getenv(name); return !(v && v[0] == '0'); }      // on unless the value starts with '0'
inline int env_int(const char* name, int dflt) { const char* v = getenv(name); return (v && v[0]) ? atoi(v) : dflt; }   // unset or empty: dflt
}  // namespace m2m
