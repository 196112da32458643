// Read log of the emulated --source plugins.  TEST INFRASTRUCTURE, force-included (-include) in front of an emitted kernel by
// tests/source_cases.py::build_emulated(read_log=True).  The emitted extra read streams (the source term, the old output of
// --time-order 2) load through __builtin_nontemporal_load; here that name becomes a function that marks every byte it reads inside one
// watched range and then performs the load.  With the range laid over `src`, the marked bytes are exactly what a launch read of it --
// loads whose values never reach a store included, which no test of values or of page protection can see.
// Not covered: --store-mask buffer (the emulated window load is a plain dereference).
#pragma once
#include <cstddef>

static const char* drs_readlog_base = nullptr;
static size_t drs_readlog_bytes = 0;
static unsigned char* drs_readlog_map = nullptr;

// watch [base, base + bytes): map[i] becomes 1 when byte i is read; map == nullptr stops the log
extern "C" void drs_readlog_watch(const void* base, size_t bytes, unsigned char* map)
{
    drs_readlog_base = (const char*)base;
    drs_readlog_bytes = bytes;
    drs_readlog_map = map;
}

template <class T> static inline T drs_readlog_load(const T* p)
{
    if (drs_readlog_map) {
        const char* c = (const char*)p;
        for (size_t i = 0; i < sizeof(T); i++)
            if (c + i >= drs_readlog_base && c + i < drs_readlog_base + drs_readlog_bytes) drs_readlog_map[c + i - drs_readlog_base] = 1;
    }
    return __builtin_nontemporal_load(p);
}
#define __builtin_nontemporal_load(p) drs_readlog_load(p)
