// tse_tables.cpp -- build_tables: the reference's edge descriptors -> every table the kernels index (tse_tables.h).  Host code
// only: tse_init uploads the result once.
#include "tse_tables.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <map>

namespace tse {

static int fail(std::string* err, const char* fmt, ...) {
  char buf[512];
  va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
  if (err) *err = buf;
  return 1;
}

static inline int edge_point(int d, int k) {  // d: 0 W, 1 E, 2 S, 3 N  (edge_mod.F90:407-422)
  switch (d) { case 0: return k * 4 + 0; case 1: return k * 4 + 3; case 2: return k; default: return 12 + k; }
}
static inline int corner_point(int d) {  // d: 4 SW, 5 SE, 6 NW, 7 NE
  switch (d) { case 4: return 0; case 5: return 3; case 6: return 12; default: return 15; }
}

namespace {
// what the descriptors say about every edge-buffer column
struct Columns {
  int maxcol = 0;
  std::vector<int> own_e, own_p, send_idx, recv_idx;
  std::vector<int> put_start, get_start, mm_recv_idx;   // first column of an edge/corner -> element
};
}  // namespace

// ---- edge descriptors -> columns, the halo slots and the compact min/max exchange
static void columns(const tse_init_args& a, Columns& C, HostTables& T) {
  const int n = a.nelemd;
  int maxcol = 0;
  for (int i = 0; i < n * 8; i++) { if (a.putmapP[i] + 4 > maxcol) maxcol = a.putmapP[i] + 4; if (a.getmapP[i] + 4 > maxcol) maxcol = a.getmapP[i] + 4; }
  for (int s = 0; s < a.nsend; s++) maxcol = std::max(maxcol, a.send_ptrP[s] - 1 + a.send_lengthP[s]);
  for (int s = 0; s < a.nrecv; s++) maxcol = std::max(maxcol, a.recv_ptrP[s] - 1 + a.recv_lengthP[s]);
  C.maxcol = maxcol;
  C.own_e.assign(maxcol, -1); C.own_p.assign(maxcol, -1); C.send_idx.assign(maxcol, -1); C.recv_idx.assign(maxcol, -1);
  C.put_start.assign(maxcol, -1); C.get_start.assign(maxcol, 0); C.mm_recv_idx.assign(maxcol, -1);
  for (int e = 0; e < n; e++)
    for (int d = 0; d < 8; d++) {
      int pm = a.putmapP[e * 8 + d];
      if (pm < 0) continue;
      C.put_start[pm] = e;
      if (d < 4) {
        for (int k = 0; k < 4; k++) {  // reversal is applied at pack time (edge_mod.F90:443-485)
          int col = pm + (a.reverse[e * 8 + d] ? 3 - k : k);
          C.own_e[col] = e; C.own_p[col] = edge_point(d, k);
        }
      } else { C.own_e[pm] = e; C.own_p[pm] = corner_point(d); }
    }
  T.ncol_send = 0;
  for (int s = 0; s < a.nsend; s++) {
    T.send_peer.push_back(a.send_peer[s]); T.send_len.push_back(a.send_lengthP[s]);
    for (int i = 0; i < a.send_lengthP[s]; i++) C.send_idx[a.send_ptrP[s] - 1 + i] = T.ncol_send++;
  }
  T.ncol_recv = 0;
  for (int s = 0; s < a.nrecv; s++) {
    T.recv_peer.push_back(a.recv_peer[s]); T.recv_len.push_back(a.recv_lengthP[s]);
    for (int i = 0; i < a.recv_lengthP[s]; i++) C.recv_idx[a.recv_ptrP[s] - 1 + i] = T.ncol_recv++;
  }
  // compact min/max exchange: one entry per (element, direction) pair that crosses the rank boundary.  Sender and
  // receiver enumerate the edge/corner start columns of a slot in increasing column order, which is the same sequence
  // on both ranks because the two slots are mirror images (the sender writes where the receiver reads).
  for (int i = 0; i < n * 8; i++) if (a.getmapP[i] >= 0) C.get_start[a.getmapP[i]] = 1;
  for (int s = 0; s < a.nsend; s++) {
    int cnt = 0;
    for (int i = 0; i < a.send_lengthP[s]; i++) {
      int col = a.send_ptrP[s] - 1 + i;
      if (C.put_start[col] >= 0) { T.mm_send_src.push_back(I2{C.put_start[col], 0}); cnt++; }
    }
    T.mm_send_len.push_back(cnt);
  }
  T.nmm_send = (int)T.mm_send_src.size();
  for (int s = 0; s < a.nrecv; s++) {
    int cnt = 0;
    for (int i = 0; i < a.recv_lengthP[s]; i++) {
      int col = a.recv_ptrP[s] - 1 + i;
      if (C.get_start[col]) { C.mm_recv_idx[col] = T.nmm_recv++; cnt++; }
    }
    T.mm_recv_len.push_back(cnt);
  }
}

// ---- the send columns' sources, the DSS gather table and the neighbour table
static int gather_tables(const tse_init_args& a, const Columns& C, HostTables& T, std::string* err) {
  const int n = a.nelemd;
  T.send_src.assign(T.ncol_send, I2{});
  for (int col = 0; col < C.maxcol; col++)
    if (C.send_idx[col] >= 0) {
      if (C.own_e[col] < 0) return fail(err, "tse_init: send column %d is written by no local element", col);
      T.send_src[C.send_idx[col]] = I2{C.own_e[col], C.own_p[col]};
    }
  auto source_of = [&](int col, I2& s) -> int {
    if (C.recv_idx[col] >= 0) { s = I2{-(C.recv_idx[col] + 2), 0}; return 0; }
    if (C.own_e[col] < 0) return 1;
    s = I2{C.own_e[col], C.own_p[col]};
    return 0;
  };
  std::vector<I2>& tab = T.dss_tab;
  std::vector<int>& nbr = T.nbr;
  tab.assign((size_t)n * 48, I2{-1, 0});
  nbr.assign((size_t)n * 8, -1);
  static const int eorder[4] = {2, 1, 3, 0};  // S, E, N, W  (edge_mod.F90:685-700)
  static const int corder[4] = {4, 5, 7, 6};  // SW, SE, NE, NW (:723-734)
  for (int e = 0; e < n; e++) {
    int cnt[16] = {0};
    for (int t = 0; t < 4; t++) {
      int d = eorder[t], gm = a.getmapP[e * 8 + d];
      if (gm < 0) return fail(err, "tse_init: element %d has no neighbour across edge %d", e, d);
      for (int k = 0; k < 4; k++) {
        I2 s;
        if (source_of(gm + k, s)) return fail(err, "tse_init: element %d edge %d reads column %d that nobody writes", e, d, gm + k);
        int p = edge_point(d, k);
        tab[((size_t)e * 16 + p) * 3 + cnt[p]++] = s;
        if (k == 0) nbr[e * 8 + d] = s.x >= 0 ? s.x : -(C.mm_recv_idx[gm] + 2);  // remote: entry of the compact min/max exchange
      }
    }
    for (int t = 0; t < 4; t++) {
      int d = corder[t], gm = a.getmapP[e * 8 + d];
      if (gm < 0) continue;
      I2 s;
      if (source_of(gm, s)) return fail(err, "tse_init: element %d corner %d reads column %d that nobody writes", e, d, gm);
      int p = corner_point(d);
      tab[((size_t)e * 16 + p) * 3 + cnt[p]++] = s;
      nbr[e * 8 + d] = s.x >= 0 ? s.x : -(C.mm_recv_idx[gm] + 2);
    }
  }
  return 0;
}

// Walk order for the DSS kernels.  Each XCD processes a contiguous range of elements (L2 is per XCD); inside
// the range we follow a greedy neighbour walk over the local element graph (west/east/south/north links) in
// strips, so that the elements whose edge values a block gathers were touched by the same XCD a few blocks
// earlier instead of a whole row of the face earlier.  Pure scheduling: results do not depend on it.
static void walk_order(int n, HostTables& T) {
  const std::vector<int>& nbr = T.nbr;
  const int S8 = (n + 7) / 8;
  std::vector<int>& order = T.order;
  order.assign(n, 0);
  constexpr int W = 8;
  for (int x = 0; x < 8; x++) {
    const int lo = x * S8, hi = std::min(n, lo + S8);
    if (lo >= hi) continue;
    std::vector<char> used(hi - lo, 0);
    int pos = lo;
    auto in = [&](int e) { return e >= lo && e < hi && !used[e - lo]; };
    for (int seed = lo; seed < hi; seed++) {
      if (used[seed - lo]) continue;
      // strip: from `seed` go east up to W elements (row segment), then continue with the northern neighbours' segment
      int rowstart = seed;
      while (rowstart >= 0 && in(rowstart)) {
        int e = rowstart, cnt = 0, first = e;
        while (e >= 0 && in(e) && cnt < W) { used[e - lo] = 1; order[pos++] = e; cnt++; int ee = nbr[e * 8 + 1]; e = ee; }
        int nn = nbr[first * 8 + 3];   // north of the segment's first element
        rowstart = nn;
      }
    }
  }
}

// Boundary-first ordering (the reference's recv_external_indices / recv_internal_indices, cuda_mod.F90:358-401): the
// elements that own a column of a send slot are computed first in every stage, so that their halo travels while
// the remaining elements are computed.  Returns the flags of the elements that touch another rank.
static std::vector<char> boundary_split(int n, HostTables& T) {
  std::vector<char> isb(n, 0);
  for (const I2& s : T.send_src) isb[s.x] = 1;
  for (const I2& s : T.mm_send_src) isb[s.x] = 1;
  for (int e = 0; e < n; e++) (isb[e] ? T.ord_bnd : T.ord_int).push_back(e);
  T.n_bnd = (int)T.ord_bnd.size(); T.n_int = (int)T.ord_int.size();
  return isb;
}

// key of a halo-ring source: local (element, point) or received column
static long ring_key(const I2& t) { return t.x >= 0 ? (long)t.x * 16 + t.y : -(long)(-(t.x + 2)) - 1; }

namespace {
// Patches: groups of neighbouring elements -- rows of up to 4 elements joined by their east links, up to 4 rows joined by
// the north link of each row's first element (no coordinates are needed and a patch may take any shape next to a cube seam or
// a rank boundary).  A DSS-on-read block owns one patch: what its slabs need from inside the patch travels through LDS, only
// the patch's halo ring comes from global memory.  Elements are taken in host order, so the patches of a full face tile it
// from its south-west corner.  The tiling is also the STORAGE order of the scratch fields (slot = patch * 16 + position).
struct Tiling {
  const HostTables& T;
  const std::vector<char>& isb;
  std::vector<std::vector<int>> patches;
  std::vector<int> pid;   // element -> patch
  Tiling(const HostTables& T_, const std::vector<char>& isb_) : T(T_), isb(isb_), pid(T_.nelemd, -1) {}

  int ring_size(const std::vector<int>& cand, int me) const {
    std::vector<long> refs;
    for (int e : cand)
      for (int i = 0; i < 48; i++) {
        const I2 t = T.dss_tab[(size_t)e * 48 + i];
        if (t.x == -1) continue;
        if (t.x >= 0 && pid[t.x] == me) continue;                       // inside the candidate (marked below)
        refs.push_back(ring_key(t));
      }
    std::sort(refs.begin(), refs.end());
    return (int)(std::unique(refs.begin(), refs.end()) - refs.begin());
  }
  int ering_size(const std::vector<int>& cand, int me) const {   // distinct elements (local or received) around the candidate
    std::vector<long> refs;
    for (int e : cand)
      for (int d = 0; d < 8; d++) {
        const int nb = T.nbr[e * 8 + d];
        if (nb == -1 || (nb >= 0 && pid[nb] == me)) continue;
        refs.push_back(nb);
      }
    std::sort(refs.begin(), refs.end());
    return (int)(std::unique(refs.begin(), refs.end()) - refs.begin());
  }
  bool fits(const std::vector<int>& cand, int me) const { return ring_size(cand, me) <= Patch::NRMAX && ering_size(cand, me) <= NER; }

  // Rank-boundary elements first, as patches of their own: a stage's first launch covers the patches that own a column of a
  // send slot (split_stage), and with the regular tiling a 4 x 4 patch is such a patch as soon as one of its elements is -- a
  // quarter of all patches on 8 ranks, for 6 % of the elements.  So up to half a patch of boundary elements is strung together
  // along the boundary (element by element over the 8-neighbourhood), and the patch is then filled with the elements right
  // behind them (edge neighbours of its members), as far as the halo ring and the element ring allow: a two-deep band along the
  // rank boundary, full patches (strips of boundary elements alone left a third of the lanes empty and cost 6 % of a step),
  // and a first launch of about twice the boundary elements' share.
  void bands() {
    const int n = T.nelemd;
    auto try_add = [&](std::vector<int>& cand, int me, int el) {
      pid[el] = me; cand.push_back(el);
      if (fits(cand, me)) return true;
      pid[el] = -1; cand.pop_back();
      return false;
    };
    for (int seed = 0; seed < n; seed++) {
      if (!isb[seed] || pid[seed] >= 0) continue;
      const int me = (int)patches.size();
      std::vector<int> cand{seed};
      pid[seed] = me;
      bool grew = true;
      while (grew && (int)cand.size() < PS / 2) {    // the chain of boundary elements
        grew = false;
        for (int back = (int)cand.size() - 1; back >= 0 && !grew; back--)
          for (int d = 0; d < 8 && !grew; d++) {
            const int nb = T.nbr[cand[back] * 8 + d];
            if (nb >= 0 && isb[nb] && pid[nb] < 0) grew = try_add(cand, me, nb);
          }
      }
      grew = true;
      while (grew && (int)cand.size() < PS) {        // the elements behind it
        grew = false;
        for (size_t i = 0; i < cand.size() && !grew; i++)
          for (int d = 0; d < 4 && !grew; d++) {
            const int nb = T.nbr[cand[i] * 8 + d];
            if (nb >= 0 && pid[nb] < 0) grew = try_add(cand, me, nb);
          }
      }
      patches.push_back(cand);
    }
  }

  // the regular tiling of the elements no band took
  void regular() {
    const int n = T.nelemd;
    for (int seed = 0; seed < n; seed++) {
      if (pid[seed] >= 0) continue;
      const int me = (int)patches.size();
      // fewer rows, then narrower rows, until the halo ring and the element ring fit the tables (one element always does)
      for (int maxrows = 4, width = 4;; ) {
        std::vector<int> cand;
        int rowstart = seed;
        for (int r = 0; r < maxrows && rowstart >= 0 && pid[rowstart] < 0; r++) {
          int e = rowstart, cnt = 0;
          const int first = e;
          while (e >= 0 && pid[e] < 0 && cnt < width) { pid[e] = me; cand.push_back(e); cnt++; e = T.nbr[e * 8 + 1]; }   // east
          rowstart = T.nbr[first * 8 + 3];                                                                             // north
        }
        if (fits(cand, me) || (maxrows == 1 && width == 1)) { patches.push_back(cand); break; }
        for (int e : cand) pid[e] = -1;
        if (maxrows > 1) maxrows--; else width--;
      }
    }
  }
};
}  // namespace

// Point order inside every slot (tse_layout.h: ppos).  An edge of an element is READ FROM OUTSIDE when the neighbour across it
// belongs to another patch (that patch's halo ring) or to another rank (the pack kernel); such an edge gets a 128-byte line of
// its own, in the order S, N, W, E.  An edge that shares a corner point with an edge placed before it (the corner elements of a
// patch export two edges) brings only its remaining points into a fresh line: it then costs its reader two lines.  The points
// nobody reads from outside fill what is left.  Slots without an element keep round 2's fixed perimeter-first order (the A/B
// of that order for every slot: profiles/r03_ab_halo_ring_bound.txt).
static void slot_point_order(const Tiling& P, HostTables& T) {
  const int n = T.nelemd;
  T.pperm.assign((size_t)T.nslots, 0x67895FEA4DCB3210ULL);
  static const int edge_dir[4] = {2, 3, 0, 1};   // S, N, W, E as direction indices (west, east, south, north = 0..3)
  for (int e = 0; e < n; e++) {
    int pos_of[16]; bool placed[16] = {false};
    int line = 0;
    for (int t = 0; t < 4; t++) {
      const int d = edge_dir[t], nb = T.nbr[e * 8 + d];
      const bool outside = nb <= -2 || (nb >= 0 && P.pid[nb] != P.pid[e]);
      if (!outside) continue;
      int cnt = 0;
      for (int k = 0; k < 4; k++) { const int pt = edge_point(d, k); if (!placed[pt]) { placed[pt] = true; pos_of[pt] = line * 4 + cnt++; } }
      if (cnt) line++;
    }
    bool used[16] = {false};
    for (int pt = 0; pt < 16; pt++) if (placed[pt]) used[pos_of[pt]] = true;
    int f = 0;
    for (int pt = 0; pt < 16; pt++) if (!placed[pt]) { while (used[f]) f++; pos_of[pt] = f; used[f] = true; }
    unsigned long long w = 0;
    for (int pt = 0; pt < 16; pt++) w |= (unsigned long long)pos_of[pt] << (4 * pt);
    T.pperm[T.slot_of[e]] = w;
  }
}

// ---- the tables of the kernels (PatchSet), and what the halo rings read from the slots (pexp)
static int patch_tables(const Tiling& P, const std::vector<char>& isb, HostTables& T, std::string* err) {
  constexpr int nrmax = Patch::NRMAX;
  const int n = T.nelemd;
  const std::vector<std::vector<int>>& pt = P.patches;
  const std::vector<int>& pid = P.pid;
  T.npatch = (int)pt.size();
  const size_t nts = (size_t)T.npatch * PS;   // table slots
  std::vector<int> tslot_of(n, -1);
  T.pslots.assign(nts, -1);
  for (int pi = 0; pi < T.npatch; pi++)
    for (size_t i = 0; i < pt[pi].size(); i++) { T.pslots[(size_t)pi * PS + i] = pt[pi][i]; tslot_of[pt[pi][i]] = pi * PS + (int)i; }
  T.pring.assign((size_t)T.npatch * nrmax, T.zero0());
  constexpr int lds_ring = Patch::LDS_RING, lds_zero = Patch::LDS_ZERO;
  T.plds.assign(nts * 48, (unsigned short)lds_zero);
  for (int pi = 0; pi < T.npatch; pi++) {
    std::map<long, int> ring;   // source -> ring entry
    for (size_t i = 0; i < pt[pi].size(); i++) {
      const int e = pt[pi][i];
      for (int k = 0; k < 48; k++) {
        const I2 t = T.dss_tab[(size_t)e * 48 + k];
        unsigned short ent = (unsigned short)lds_zero;
        if (t.x >= 0 && pid[t.x] == pi) ent = (unsigned short)lds_own_entry(tslot_of[t.x] - pi * PS, t.y);
        else if (t.x != -1) {
          const long key = ring_key(t);
          auto it = ring.find(key);
          if (it == ring.end()) {
            if ((int)ring.size() >= nrmax) return fail(err, "tse_init: halo ring of patch %d exceeds %d entries", pi, nrmax);
            it = ring.emplace(key, (int)ring.size()).first;
            T.pring[(size_t)pi * nrmax + it->second] = t.x >= 0 ? (unsigned)T.slot_of[t.x] * 16 + ppos(T.pperm[T.slot_of[t.x]], t.y) : T.halo0() + (unsigned)(-(t.x + 2));
          }
          ent = (unsigned short)(lds_ring + it->second);
        }
        T.plds[((size_t)pi * PS + i) * 48 + k] = ent;
      }
    }
  }
  for (unsigned ent : T.pring)   // what the halo rings read from the slots
    if (ent < (unsigned)T.nslots * 16) T.pexp[ent / 16] = std::max<unsigned char>(T.pexp[ent / 16], (unsigned char)((ent % 16) / 4 + 1));
  // element ring and neighbour entries of every patch, for the bounds image of the stage-3 kernel (k_advance<2,3>)
  T.pering.assign((size_t)T.npatch * NER, 0);
  T.pnb.assign(nts * 8, 255);
  for (int pi = 0; pi < T.npatch; pi++) {
    std::map<int, int> ring;   // element (or -(received entry) - 2) -> ring entry
    for (int r = 0; r < NER; r++) T.pering[(size_t)pi * NER + r] = pt[pi][0];   // unused entries: any valid element
    for (size_t i = 0; i < pt[pi].size(); i++) {
      const int e = pt[pi][i];
      for (int d = 0; d < 8; d++) {
        const int nb = T.nbr[e * 8 + d];
        if (nb == -1) continue;
        if (nb >= 0 && pid[nb] == pi) { T.pnb[((size_t)pi * PS + i) * 8 + d] = (unsigned char)(tslot_of[nb] - pi * PS); continue; }
        auto it = ring.find(nb);
        if (it == ring.end()) {
          if ((int)ring.size() >= NER) return fail(err, "tse_init: patch %d has more than %d elements around it", pi, NER);
          it = ring.emplace(nb, (int)ring.size()).first;
          T.pering[(size_t)pi * NER + it->second] = nb >= 0 ? nb : n + (-(nb + 2));
        }
        T.pnb[((size_t)pi * PS + i) * 8 + d] = (unsigned char)(PS + it->second);
      }
    }
  }
  // rank-boundary patches first, as the elements above
  for (int pi = 0; pi < T.npatch; pi++) {
    bool b = false;
    for (int e : pt[pi]) b = b || isb[e];
    (b ? T.plist_bnd : T.plist_int).push_back(pi);
  }
  T.np_bnd = (int)T.plist_bnd.size(); T.np_int = (int)T.plist_int.size();
  return 0;
}

// ---- the send columns in slot space, the DSS contributions as chunk entries, the remap's block lists
static void slot_space(const std::vector<char>& isb, HostTables& T) {
  const int n = T.nelemd;
  T.send_src_s = T.send_src;
  for (I2& t : T.send_src_s) { t.x = T.slot_of[t.x]; t.y = ppos(T.pperm[t.x], t.y); }   // {slot, position within the slot}
  for (const I2& t : T.send_src_s) T.pexp[t.x] = std::max<unsigned char>(T.pexp[t.x], (unsigned char)(t.y / 4 + 1));   // what the pack kernel reads
  // the same contributions per ELEMENT as global entries of a chunk, for the remap that assembles the last DSS of a cycle on read
  T.etab.resize((size_t)n * 48);
  for (size_t i = 0; i < T.etab.size(); i++) {
    const I2 t = T.dss_tab[i];
    T.etab[i] = t.x >= 0 ? (unsigned)T.slot_of[t.x] * 16 + ppos(T.pperm[T.slot_of[t.x]], t.y) : t.x == -1 ? T.zero0() : T.halo0() + (unsigned)(-(t.x + 2));
  }
  // the remap's block lists: all / rank-boundary / interior elements in slot order (patch by patch)
  std::vector<int>& by_slot = T.rl_all;
  by_slot.resize(n);
  for (int e = 0; e < n; e++) by_slot[e] = e;
  std::sort(by_slot.begin(), by_slot.end(), [&](int x, int y) { return T.slot_of[x] < T.slot_of[y]; });
  for (int e : by_slot) (isb[e] ? T.rl_bnd : T.rl_int).push_back(e);
}

int build_tables(const tse_init_args& a, bool strips, HostTables* out, std::string* err) {
  HostTables& T = *out;
  T = HostTables();
  const int n = T.nelemd = a.nelemd;
  Columns C;
  columns(a, C, T);
  if (gather_tables(a, C, T, err)) return 1;
  walk_order(n, T);
  const std::vector<char> isb = boundary_split(n, T);   // elements that touch another rank
  Tiling P(T, isb);
  // strips (TSE_BOUNDARY_STRIPS=1): rank-boundary elements in patches of their own (Tiling::bands).  Off by default: on 8 ranks of
  // ne120 it halves the first launch of a stage (25.8 -> 11.8 % of the patches) but the ragged tiling behind the band costs 3 % of
  // a rank's step (12.6 -> 13.0 ms in the loopback rehearsal, profiles/r03_ab_boundary_bands.txt), and the first launch only
  // matters where an exchange outlasts the interior launch -- 0.7 ms of xGMI transfer against 1.3-2.2 ms of interior work here.
  if (strips) P.bands();
  P.regular();
  // ---- storage
  T.nslots = (int)P.patches.size() * PS;
  T.slot_of.assign(n, -1);
  for (size_t pi = 0; pi < P.patches.size(); pi++)
    for (size_t i = 0; i < P.patches[pi].size(); i++) T.slot_of[P.patches[pi][i]] = (int)pi * PS + (int)i;
  T.cse = (unsigned)(T.nslots + 1) * 16 + (unsigned)std::max(0, T.ncol_recv);
  slot_point_order(P, T);
  // lines of a slot that k_lap1<1> must store: 1 + the last line that holds a point some patch's halo ring or a
  // send column reads -- taken from those tables themselves (patch_tables, slot_space), so that it covers corner-only readers and
  // irregular patches too; the per-slot order packs the exported edges into the first lines, so this is a quarter of the field on average
  T.pexp.assign((size_t)T.nslots, 0);
  if (patch_tables(P, isb, T, err)) return 1;
  slot_space(isb, T);
  return 0;
}

// the wording of a column fault (tse_remap_check.h), for check_remap_grids and for the device-side check of tse_remap_view
std::string remap_grid_message(int e, int p, const RemapGridFault& f, bool mean) {
  const char* what = "";
  switch (f.code) {
    case REMAP_GRID_SRC: what = "dp1 is not a finite positive number: dp1"; break;
    case REMAP_GRID_SRC_SUM:
      what = f.has_limit ? "sum(dp1) is so large that sum(dp1) + 1 == sum(dp1), the search of the last level cannot end: sum(dp1)"
                                : "sum(dp1) is not finite: sum(dp1)";
      break;
    case REMAP_GRID_TGT: what = mean ? "dp2 is zero, negative or not finite (a layer mean is divided by it): dp2" : "dp2 is negative or not finite: dp2"; break;
    case REMAP_GRID_TGT_SUM: what = "the target grid leaves the source column: partial sum of dp2"; break;
  }
  // Every message ends on the limit, "nan" where the fault has none: the text check_remap_grids has always produced (its `lim == lim`
  // was compiled away under -fno-honor-nans), kept to the letter because callers match on it.
  std::string msg;
  fail(&msg, "%s = %.17g at element %d, column %d, level %d (counted from 0); sum(dp1) + 1 = %.17g", what, f.value, e, p, f.level,
       f.has_limit ? f.limit : std::nan(""));
  return msg;
}

int check_remap_grids(const double* dp1, const double* dp2, int nelem, int nlev, int* where, std::string* err) {
  if (!dp1 || !dp2 || nelem < 0 || nlev < 1) return fail(err, "remap grids: null argument or bad size (nelem = %d, nlev = %d)", nelem, nlev);
  for (int e = 0; e < nelem; e++)
    for (int p = 0; p < 16; p++) {
      RemapGridFault f;   // the column test itself is shared with the device (tse_remap_check.h)
      if (remap_column_check(dp1 + (size_t)e * nlev * 16 + p, 16, dp2 + (size_t)e * nlev * 16 + p, 16, nlev, false, &f)) {
        if (where) { where[0] = e; where[1] = p; where[2] = f.level; }
        return fail(err, "%s", remap_grid_message(e, p, f, false).c_str());
      }
    }
  return 0;
}

}  // namespace tse
