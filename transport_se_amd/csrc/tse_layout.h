// tse_layout.h -- the constants and index helpers of the device layout that host and device code share: the kernels
// (tse_device.h, tse_kernels.h) and the table builder (tse_tables.cpp, plain host C++17: no HIP header).
#pragma once
#include <cstddef>

#ifndef __HIP__   // a host compiler: the qualifiers of the shared helpers mean nothing there
#define __host__
#define __device__
#define __forceinline__ inline __attribute__((always_inline))
#endif

#define NP 4
// The level count is a build-time setting, as the reference's PLEV (dimensions_mod.F90:27): a build may pass -DNLEV=<n>
// (NLEVP follows).  The default is 72.  The static_asserts of the kernels name the rules, which together allow the multiples of
// 8 from 16 to 72 and 80 (tse_kernels.h: the remap's blocks of 8 levels and its two elements per CU -- one at 80); anything else
// fails to compile.  Those values compile; 72, 64 and 80 are the ones built and tested.
#ifndef NLEV
#define NLEV 72
#endif
#ifndef NLEVP
#define NLEVP (NLEV + 1)
#endif
static_assert(NLEVP == NLEV + 1, "NLEVP = NLEV + 1");

namespace tse {

// Scratch layout: CL levels per chunk.  The DSS-on-read kernels work on blocks of (patch of 16 element slots) x (one chunk):
// 16 slots x 4 levels x 4 rows = 256 lanes, and a slot's 16 points x 4 levels are 512 contiguous bytes.
constexpr int CL = 4;
constexpr int NCHUNK = NLEV / CL;
static_assert(NLEV % CL == 0 && CL % 2 == 0, "chunks hold whole level pairs: NLEV must be a multiple of 4");
constexpr int PS = 16;        // element slots per patch (4 x 4 elements): slot = patch * PS + position
// Block shape of the DSS-on-read kernels: a block owns a patch of PS element slots, 256 lanes; its tables (PatchSet, tse_tables.cpp)
// name the storage slot of every element and of every halo-ring entry.  (Wider blocks of 6 x 4 and 8 x 4 elements have a shorter
// ring per element but cost occupancy: 3.4 and 8.5 ms per step more, same bits -- profiles/r03_ab_patch_shapes.txt; retired.)
struct Patch {
  static constexpr int THREADS = PS * 16;
  // halo-ring entries (distinct (element, point) pairs outside the patch: 68 for a full patch; tse_tables.cpp gives a patch fewer
  // rows if its ring would not fit); lanes 2r, 2r+1 load entry r
  static constexpr int NRMAX = 96;
  // Entries of one LDS buffer (an entry = the CL levels of a point = 32 bytes = 8 of the 64 banks): the own points, the ring, one all-zero
  // entry.  The own points are SKEWED (lds_own_entry): a slot takes LDS_SLOT = 20 entries instead of 16, and point (j, i) of a slot sits at
  // position 4j + ((i + j) & 3).  A wave reads, in one ds_read_b64, the same edge of four slots (its rows' neighbour values): in the
  // natural order an east or west edge is points 3,7,11,15 / 0,4,8,12 -- two bank groups -- and the four slots, 512 bytes apart, fall on
  // the same two: 8 cycles for the 2 the 512 bytes need.  Skewed, the four points of any edge are in four different groups and slots
  // s, s+1 in complementary halves of the banks: 2 cycles.  (SQ_LDS_BANK_CONFLICT: more than half of the LDS cycles of the four
  // gathering kernels before; profiles/r03_ab_lds_skew.txt.)
  static constexpr int LDS_SLOT = 20;
  static constexpr int LDS_RING = PS * LDS_SLOT, LDS_ZERO = LDS_RING + NRMAX, LDS_ENT = LDS_ZERO + 1;
  static_assert(2 * NRMAX <= THREADS, "one 16-byte ring load per lane");
};
__host__ __device__ inline int lds_own_entry(int sl, int p) { return sl * Patch::LDS_SLOT + (p & ~3) + (((p & 3) + (p >> 2)) & 3); }
// Inside a slot the 16 points are stored in a PER-SLOT order (nibble p of the slot's 64-bit word pperm[slot] = position of
// point p).  The memory system moves whole 128-byte lines (tools/fetch_probe.hip: 32 bytes out of every line cost what the
// line costs), a position holds the CL = 4 levels of a point = 32 bytes, so a slot is four lines of four points -- and what a
// neighbouring patch's halo ring reads from a slot is one EDGE of the element (4 points).  tse_init gives every edge that
// some patch or neighbour rank reads a line of its own (slot_point_order, tse_tables.cpp), so a ring edge is one line instead of the
// two that three of the four edges straddled with one fixed perimeter-first order.
__host__ __device__ __forceinline__ int ppos(unsigned long long perm, int p) { return (int)((perm >> (4 * p)) & 15ull); }
// qmin/qmax(k,q,e) of prim_advection_mod (:459) in the device layout [e][k / CL][q][k % CL]
// (the tracer count of the bounds layout is rounded up to a multiple of 4: the 4 levels of 4 consecutive tracers are one aligned
// 128-byte line, so that the kernels that emit bounds can write whole lines)
__host__ __device__ __forceinline__ int mm_qpad(int qsize) { return (qsize + 3) & ~3; }
constexpr int NER = 48;            // elements around a patch whose bounds the stage-3 kernel reads (a full patch: 20; a two-deep band
                                   // along a rank boundary: every received (element, direction) pair is an entry of its own, about 40)

}  // namespace tse
