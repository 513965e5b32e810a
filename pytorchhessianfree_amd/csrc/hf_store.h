// hf_store.h -- the one definition of the stores that hand data to the next launch of an iteration graph (chain
// stores), and the compile-time switch of each kernel family that uses them.  Self-contained: hf_unpack.h and
// hf_common.h include it.  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

// ---------------------------------------------------------------------------
// chain stores.  One PCG iteration is one graph of dependent launches; whatever a launch writes is read by the next
// one, possibly on another XCD, so every dirty L2 line a kernel leaves behind is written back at its end, before the
// consumer may start.  A write-through (sc1) store moves that write-back into the kernel, where it overlaps the work
// of the other workgroups.  Only the cache policy differs: no fence, flag or drain is added, the kernel's end is
// still the release, and with the switch at 0 the store is the plain store (same instructions as without this helper).
// One compile-time switch per kernel family (A/B: -DHF_WT_CONV=.. -DHF_WT_ELEM=.. -DHF_WT_VEC=..):
//   CONV  split-K slabs / single-split outputs and BatchNorm partial rows of the convolutions (hf_conv.hip);
//   ELEM  what the elementwise, pooling and head kernels write for the next launch (hf_bn.hip, hf_head.hip);
//   VEC   the parameter-sized vectors: gather / scatter (hf_pack.hip, hf_unpack.h) and K2 / K3 (hf_pcg.hip).
// Whole-bench gate on one MI355X, three alternating runs per variant (profiles/r22_*): CONV is
// on (its lowest run above the highest run without it, twice); ELEM, VEC and either half of VEC alone were inside
// the noise of the build without them or below it, and stay off.
//
// The 16-byte form is issued from inline assembly, and the compiler does not count such a store: the s_waitcnt it puts
// in front of a barrier or a fence does not cover it.  A kernel that writes lines with chain_store16 and then, in the
// same launch, stores to or loads from those lines again from other lanes (behind a barrier), or signals them to
// another workgroup, spells out `s_waitcnt vmcnt(0)` itself first (k_pack's zero stream does).  A kernel whose stores
// are only read by later launches needs nothing: the kernel's end waits for them.
// ---------------------------------------------------------------------------
#ifndef HF_WT_CONV
#define HF_WT_CONV 1
#endif
#ifndef HF_WT_ELEM
#define HF_WT_ELEM 0
#endif
#ifndef HF_WT_VEC
#define HF_WT_VEC 0
#endif

namespace hf_shared {

// 4- and 8-byte values (float, double)
template <bool WT, typename T>
__device__ __forceinline__ void chain_store(T* p, T v) {
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "one dword or one dwordx2");
  if constexpr (WT) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *p = v;
}

// one aligned 16-byte value (float4, double2, a quad of floats) as ONE store: four narrow write-through stores of
// the same bytes cost several times the one wide store.  p points to global memory.  The trailing s_nop keeps the
// compiler's next instruction off the data registers until the store has read them.
template <bool WT, typename V>
__device__ __forceinline__ void chain_store16(V* p, const V& v) {
  static_assert(sizeof(V) == 16 && alignof(V) == 16, "one aligned dwordx4");
  if constexpr (WT) {
    typedef float Raw __attribute__((ext_vector_type(4)));
    Raw r;
    __builtin_memcpy(&r, &v, 16);
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(p), "v"(r) : "memory");
  } else {
    *p = v;
  }
}

}  // namespace hf_shared
