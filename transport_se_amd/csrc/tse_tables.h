// tse_tables.h -- the host tables tse_init derives from the reference's edge descriptors (putmapP/getmapP/reverse + the
// Send/RecvCycle slots): gather and neighbour tables, halo column maps, walk orders, the patch tiling and its tables.  A pure
// function of the descriptors, in plain host C++ (no HIP runtime): tse_init uploads the result, the hooks library hands it to
// the CPU tests (tse_test_tables).
#pragma once
#include <string>
#include <vector>

#include "../../include/transport_se_hip.h"
#include "tse_layout.h"
#include "tse_remap_check.h"

namespace tse {

// a source entry {x, y} of the gather tables; uploaded as int2
struct I2 { int x, y; };
static_assert(sizeof(I2) == 8 && offsetof(I2, y) == 4, "laid out as int2");

struct HostTables {
  int nelemd = 0;
  // halo: one slot per neighbour rank; kind 0: edge-buffer columns per slot, kind 1: (element, direction) pairs of the compact
  // min/max exchange
  int ncol_send = 0, ncol_recv = 0, nmm_send = 0, nmm_recv = 0;
  std::vector<int> send_peer, recv_peer, send_len, recv_len, mm_send_len, mm_recv_len;
  std::vector<I2> send_src;      // [ncol_send] {element, point} a send column is packed from
  std::vector<I2> mm_send_src;   // [nmm_send] {element, 0} of a min/max send entry
  std::vector<I2> dss_tab;       // [e][16][3] {source element (>= 0 local, -1 none, <= -2 received column -(v+2)), source point}
  std::vector<int> nbr;          // [e][8] neighbour element across direction d (>= 0 local, -1 none, <= -2 received min/max entry -(v+2))
  std::vector<int> order;        // walk order of the DSS kernels (per XCD)
  std::vector<int> ord_bnd, ord_int;   // elements that touch another rank / that do not
  int n_bnd = 0, n_int = 0;
  // the patch tiling, also the storage order of the scratch fields (slot = patch * PS + position)
  int nslots = 0;
  unsigned cse = 0;                      // entries (points, halo columns) per chunk of a scratch plane
  std::vector<int> slot_of;              // [e]
  std::vector<unsigned long long> pperm; // [slot] point order inside the slot (ppos)
  std::vector<unsigned char> pexp;       // [slot] lines of the slot that hold points read from outside its patch
  std::vector<I2> send_src_s;            // the send columns in slot space: {slot, position within the slot}
  std::vector<unsigned> etab;            // [e][16][3] dss_tab as entries within a chunk
  std::vector<int> rl_all, rl_bnd, rl_int;   // all / rank-boundary / interior elements in slot order
  // the tables of the DSS-on-read kernels (PatchSet)
  int npatch = 0, np_bnd = 0, np_int = 0;
  std::vector<int> pslots;               // [patch][PS] element (-1: empty)
  std::vector<unsigned> pring;           // [patch][NRMAX] ring entry -> entry index within a chunk
  std::vector<unsigned short> plds;      // [patch][PS][48] LDS entry of every contribution
  std::vector<int> pering;               // [patch][NER] elements around the patch (>= nelemd: received entry nelemd + i)
  std::vector<unsigned char> pnb;        // [patch][PS][8] neighbour as patch position (< PS) or PS + element-ring entry; 255: none
  std::vector<int> plist_bnd, plist_int; // patches that hold a rank-boundary element / that do not
  unsigned zero0() const { return (unsigned)nslots * 16; }          // entry index of the zero slot within a chunk
  unsigned halo0() const { return (unsigned)(nslots + 1) * 16; }    // entry index of halo column 0
};

// strips: TSE_BOUNDARY_STRIPS (rank-boundary elements in patches of their own).  Returns 0, or 1 with the reason in *err.
int build_tables(const tse_init_args& a, bool strips, HostTables* out, std::string* err);

// The precondition of remap_Q_ppm's bracket search (k_remap: `while (pio(kk) <= pin(k+1)) kk++`), checked on the host before anything
// reaches the device.  dp1, dp2: [e][nlev][16].  Per column, in the kernel's serial order, pio(k+1) = pio(k) + dp1(k) and
// pin(k+1) = pin(k) + dp2(k) from 0; the search of level k < nlev ends only at pio(nlev+2) = pio(nlev+1) + 1, so it needs
// pin(k+1) < pio(nlev+1) + 1; the last level uses pin(nlev+1) = pio(nlev+1) itself, so it needs pio(nlev+1) + 1 > pio(nlev+1) in
// fp64, i.e. sum(dp1) < 2^53.  Refused: a dp1 that is not a finite positive number, a column whose sum(dp1) + 1 does not exceed
// sum(dp1), a dp2 that is negative or not finite, a partial sum of dp2 below the last level that is >= sum(dp1) + 1 (both in fp64).
// Returns 0, or 1 with the first offender in scan order (element, then column, then level; all counted from 0) in where[3] (if
// given) and in *err.
// The test of one column is remap_column_check (tse_remap_check.h), which the device runs too (tse_remap_view).
int check_remap_grids(const double* dp1, const double* dp2, int nelem, int nlev, int* where, std::string* err);
// the message of a column fault in check_remap_grids' wording (mean: the zero target layer a layer-mean field refuses)
std::string remap_grid_message(int e, int p, const RemapGridFault& f, bool mean);

}  // namespace tse
