// phase_trace.h -- the in-kernel phase trace of the three spatially tiled fused kernels (resblock.hip, csp_stage.hip, stem_down.hip).
// Kernel experiments only (scripts/build_variant.sh with -DRB_TRACE=128|64, -DCS_TRACE=1 or -DSD_TRACE=1; read out by
// scripts/phase_trace.py): chosen waves stamp s_memtime at numbered points of a few tiles / output rows.  A kernel keeps what is its
// own -- the __device__ buffer and its shape, `tr_t[]`, the `tr_on` condition that picks workgroup and tiles, the point numbers and
// the write-out -- and takes from here the stamp and the host-side reader.  Without a *_TRACE macro both expand to nothing.
#pragma once

#if defined(RB_TRACE) || defined(CS_TRACE) || defined(SD_TRACE)
// stamp point P of this wave (`tr_on`, `tr_t` are the kernel's); pinned so that nothing is scheduled across the stamp
#define PHASE_POINT(P)                                                                                      \
    do {                                                                                                    \
        __builtin_amdgcn_sched_barrier(0);                                                                  \
        if (tr_on) asm volatile("s_memtime %0" : "=s"(tr_t[P]));                                            \
        __builtin_amdgcn_sched_barrier(0);                                                                  \
    } while (0)
// exported `int NAME(unsigned long long* dst)`: copies the whole trace buffer BUF (a __device__ array of the enclosing namespace) out
#define PHASE_TRACE_READER(NAME, BUF) \
    extern "C" int NAME(unsigned long long* dst) { return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(BUF), sizeof(BUF)); }
#else
#define PHASE_POINT(P)
#define PHASE_TRACE_READER(NAME, BUF)
#endif
