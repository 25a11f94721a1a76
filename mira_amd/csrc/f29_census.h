// TEST-ONLY (F29_TRACK builds: the CPU emulation and the host tests of tests/emu): the branch census of the group law.  F29_HIT /
// F29_REGION (field29.cuh) and HOSTF_HIT / HOSTF_REGION (host_field.hpp) count every exit of the point additions and doublings
// under (running kernel, section of it, function, exit).  The emulation's launch macros (tests/emu/emu.h) name the kernel on
// every thread that runs its lanes; any other thread -- the caller between launches, the library's host threads -- counts under
// "host".  Kernel and section are per thread and scoped: a section lasts until the end of the block that opened it and then
// gives way to the one around it, so a hit outside every marked function has the empty section.  mira_emu_census_read /
// mira_emu_census_reset (capi.hip, in libmira_emu.so alone) read and clear the table.  Never part of libmira_gpu.so.
#pragma once
#include <cstdint>
#include <map>
#include <mutex>
#include <tuple>

struct EmuCensus {
    std::mutex m;
    std::map<std::tuple<const char *, const char *, const char *, const char *>, uint64_t> hits;   // keyed by the literals' addresses: merged by text when read
};
inline EmuCensus emu_census;
inline thread_local const char *emu_kernel = "host";
inline thread_local const char *emu_region_name = "";
inline void emu_hit(const char *fn, const char *site) {
    std::lock_guard<std::mutex> lk(emu_census.m);
    emu_census.hits[std::make_tuple(emu_kernel, emu_region_name, fn, site)]++;
}
struct EmuKernelScope {                                      // one per thread that runs lanes of a launch
    const char *kernel_before, *region_before;
    explicit EmuKernelScope(const char *name) : kernel_before(emu_kernel), region_before(emu_region_name) { emu_kernel = name; emu_region_name = ""; }
    ~EmuKernelScope() { emu_kernel = kernel_before; emu_region_name = region_before; }
    EmuKernelScope(const EmuKernelScope &) = delete;
    EmuKernelScope &operator=(const EmuKernelScope &) = delete;
};
struct EmuRegionScope {
    const char *before;
    explicit EmuRegionScope(const char *name) : before(emu_region_name) { emu_region_name = name; }
    ~EmuRegionScope() { emu_region_name = before; }
    EmuRegionScope(const EmuRegionScope &) = delete;
    EmuRegionScope &operator=(const EmuRegionScope &) = delete;
};
#define EMU_CENSUS_CAT2(a, b) a##b
#define EMU_CENSUS_CAT(a, b) EMU_CENSUS_CAT2(a, b)
#define EMU_REGION_SCOPE(name) EmuRegionScope EMU_CENSUS_CAT(emu_region_scope_, __LINE__)(name)
