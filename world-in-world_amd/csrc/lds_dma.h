// LDS-DMA, wait and barrier helpers shared by the kernels that fill LDS with global_load_lds (include after common.h).
// Forms that differ per kernel stay in their files: temporal.hip's base + 32-bit offset glds16, temporal32.hip's and
// ffn32.hip's variants, the two wait_vmcnt_rt switches (they clamp differently) and the per-file dump sinks.
#pragma once
#include "common.h"

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

// LDS-DMA through the builtin: 16 bytes per lane from a per-lane address, LDS destination = wave-uniform base + 16 * lane
WIW_DEV void glds16(const char* g, char* l) { __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)l, 16, 0, 0); }

// The same transfer as INLINE ASM, for kernels that keep ds_reads in flight next to pending DMA.  hipcc models the builtin
// as a FLAT access that may touch LDS: while one is pending every compiler-inserted wait for a ds_read is lgkmcnt(0)
// (ffn.hip: the Y-waves' software-pipelined fragment reads of phase 2, 8 in flight, would drain at every use), and it puts
// `s_waitcnt vmcnt(0)` in front of the next LDS read it cannot prove disjoint (temporal.hip: the epilogue's fold-vector
// reads waited ~1 000 cycles for the next item's prefetch that had just been issued, r06c trace).  The asm form is invisible
// to that bookkeeping: its completion is counted by hand (wait_vmcnt below), exactly as for the builtin.  M0 carries the
// LDS address and is saved / restored inside the statement (the compiler does not preserve it around asm).
WIW_DEV void glds16_asm(const char* g, uint32_t lds_addr) {
    const uint32_t lds = __builtin_amdgcn_readfirstlane(lds_addr);
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(g), "s"(lds) : "memory");
}
WIW_DEV void glds16_asm(const char* g, char* l) { glds16_asm(g, (uint32_t)(uintptr_t)(lptr_t)l); }

template <int N>
WIW_DEV void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

WIW_DEV void wave_lds_sync() {   // order this wave's LDS writes before its following LDS reads (and vice versa)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
WIW_DEV void slot_barrier() {   // close a slot: this wave's LDS accesses are retired, then rendezvous of the block's waves
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}

WIW_DEV wiw_f32x2 pk_fma(wiw_f32x2 a, wiw_f32x2 b, wiw_f32x2 c) { return __builtin_elementwise_fma(a, b, c); }   // v_pk_fma_f32

// One K tile forward in the implicit-GEMM K walk of gemm.hip / gemm_huge.hip (see the cursor declaration in the kernels):
// tap-major, or channel-block major under WIW_K_CMAJOR; the fused shortcut segment (tap 9, conv3x3 only) is walked last in both.
struct WiwKCur { int tap, cc; };
template <int MODE, int KT>
WIW_DEV WiwKCur wiw_advance_k(WiwKCur c, const int Ctot, const bool cmajor) {   // by value: by-reference cursors end up in scratch
    int ld_tap = c.tap, ld_cc = c.cc;
    constexpr int NT = MODE == WIW_A_CONV_T3 ? 3 : 9;
    if (MODE != WIW_A_DENSE && cmajor && !(MODE == WIW_A_CONV3X3 && ld_tap == 9)) {
        if (++ld_tap == NT) {
            ld_tap = 0;
            ld_cc += KT;
            if (MODE == WIW_A_CONV3X3 && ld_cc == Ctot) { ld_tap = 9; ld_cc = 0; }   // (only reached with a shortcut segment)
        }
    } else {
        ld_cc += KT;
        if (ld_cc == Ctot && !(MODE == WIW_A_CONV3X3 && ld_tap == 9)) { ld_cc = 0; ++ld_tap; }
    }
    return WiwKCur{ld_tap, ld_cc};
}
