// Shared by the units of the CPU emulation library (libapsu_he_hostemu.so), one per kernel family.  The library steps the SAME pure
// headers the gfx950 kernels run over every lane of a launch, for the no-GPU test tier.  It is NOT a fallback path: nothing in it is
// reachable from the C ABI, and only tests load it (tests/emu_lib.py).
#pragma once
#include <exception>
#include <string>

inline thread_local std::string g_err;          // the text of the calling thread's last refusal
extern "C" const char *emu_last_error();        // (rules.cpp)

// fn(), or -1 with the exception's text left in emu_last_error
template <class F> auto guarded(F &&fn) -> decltype(fn())
{
    try { return fn(); } catch (const std::exception &e) { g_err = e.what(); return -1; }
}
