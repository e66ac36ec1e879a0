// Device helpers shared by the Conv2D backprop-filter kernels that stage NHWC
// tiles with global_load_lds and transpose on the LDS read (conv_dw_tall.hip,
// conv_dw_wide.hip).
#pragma once

#include "hip_common.h"

namespace stf_dw {

typedef short v4s __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------
// Transposing fragment read. ds_read_b64_tr_b16 works on blocks of 16 lanes:
// lane L of a block supplies the address of 4 consecutive 16-bit elements,
// and lane i receives, as element j, element i % 4 of what lane 4*j + i / 4
// supplied. With lane L pointing at rows 4*(L % 4)..+3 of k index L / 4, lane
// i ends up with row i at k = 0..3. Two reads give the 8 consecutive k that
// v_mfma_f32_16x16x32_bf16 wants from lane (row = lane % 16, k group =
// lane / 16): FragK is the k index and FragRow the first of the 4 rows whose
// address this lane supplies for half h; FragTr(p0, p1) reads the fragment.
// ---------------------------------------------------------------------------
__device__ __forceinline__ int FragK(int lane, int h) {
  return (lane >> 4) * 8 + h * 4 + ((lane >> 2) & 3);
}
__device__ __forceinline__ int FragRow(int lane) { return (lane & 3) * 4; }

__device__ __forceinline__ bf16x8 FragTr(const uint16_t* p0,
                                         const uint16_t* p1) {
  v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) v4s*)p0);
  v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) v4s*)p1);
  s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, v);
}

// One 16-byte global_load_lds per lane: LDS slot i of the 64 slots at `l`
// (wave-uniform) comes from lane i's address g. Written as assembly so that
// the compiler does not count it: it would otherwise drain vmcnt before
// every LDS read of another buffer. The kernel counts and waits itself
// (WaitLoads). m0 is reserved and cannot be named as a
// clobber; nothing else in these kernels uses it.
__device__ __forceinline__ void Glds16(const uint16_t* g, uint16_t* l) {
  uint32_t m0 = __builtin_amdgcn_readfirstlane(
      (uint32_t)(size_t)(__attribute__((address_space(3))) uint16_t*)l);
  asm volatile(
      "s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off"
      :
      : "s"(m0), "v"(g)
      : "memory");
}

// s_waitcnt takes an immediate: wait until at most n loads are outstanding
// (n is wave-uniform; an n outside the table waits for all of them).
__device__ __forceinline__ void WaitLoads(int n) {
  switch (n) {
#define STF_WAIT_CASE(N) \
  case N: asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory"); break;
    STF_WAIT_CASE(1) STF_WAIT_CASE(2) STF_WAIT_CASE(3) STF_WAIT_CASE(4)
    STF_WAIT_CASE(5) STF_WAIT_CASE(6) STF_WAIT_CASE(7) STF_WAIT_CASE(8)
    STF_WAIT_CASE(9) STF_WAIT_CASE(10) STF_WAIT_CASE(11) STF_WAIT_CASE(12)
#undef STF_WAIT_CASE
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
}

}  // namespace stf_dw
