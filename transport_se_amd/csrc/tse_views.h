// tse_views.h -- the descriptor logic of the strided device views (tse_view_put / tse_view_get / tse_view_plan): which fields a view may
// name in which direction, their extents and their dense internal layout, the conversion path a set of strides takes, its footprint and
// the overlap test of a destination view.  Plain host C++ (tse_views.cpp: no HIP header); tse_views_api.hip adds the checks that need the
// device and launches the kernels of tse_view_kernels.h.
#pragma once
#include <cstdint>
#include <string>

#include "../../include/transport_se_hip.h"
#include "tse_layout.h"

namespace tse {

enum ViewField { VF_QDP, VF_VN0, VF_DP, VF_ETA, VF_OMEGA_P, VF_DIVDP, VF_DIVDP_PROJ, VF_DP3D, VF_PS_V, VF_Q, VF_LNPS };

// axes in the order of tse_view::stride: element, q, level, j, i
struct ViewPlan {
  int field = 0;          // ViewField
  int path = 0;           // 0 point-fastest, 1 level-fastest, 2 generic
  int ext[5] = {0};       // extent of every axis of the view (1 for an axis the field does not have)
  long long lib[5] = {0}; // strides (doubles) of the library's dense array: vn0 is [e][k][c][p], eta_dot_dpdn has NLEVP levels per element
  long long lo = 0, hi = 0;   // footprint [lo, hi) of the view in doubles relative to ptr
};

// The addresses a view or a dense range may touch, [lo, hi) in bytes: a view's are its ptr and the footprint of its plan, in 128 bits (a
// stride may carry the sum below zero or past 2^64).  The one statement of "meets" and "inside" for every overlap and allocation rule.
struct Footprint {
  __int128 lo, hi;
  Footprint(const tse_view* v, const ViewPlan& p) : lo((__int128)(uintptr_t)v->ptr + (__int128)p.lo * 8), hi((__int128)(uintptr_t)v->ptr + (__int128)p.hi * 8) {}
  Footprint(const void* base, size_t bytes) : lo((__int128)(uintptr_t)base), hi(lo + (__int128)bytes) {}
  bool meets(const Footprint& o) const { return lo < o.hi && o.lo < hi; }   // (touching is disjoint)
  bool inside(const Footprint& o) const { return lo >= o.lo && hi <= o.hi; }
};

// Whether a kernel may move 16 bytes per lane on the view side: on path 0 the double2 parts of every (e, q, k) slab, on path 1 the level
// pairs of every row of every (e, q) tile.  The base 16-byte aligned, the element and q strides even, and the stride between the units
// even: the level stride on path 0, the i stride (the pitch of the rows) on path 1.  Never on path 2.  The one statement of the rule:
// every launch of a kernel with a WIDE parameter asks here (tse_view_launch.h: with_view_path).  It does not see the extents, so it also
// refuses a view whose only odd stride belongs to an axis of extent 1.
bool view_wide(int path, const tse_view* v);

// Returns 0, or 1 with the reason in *err (a refused axis is named).
int view_plan(const char* field, int nelemd, int qsize, const tse_view* v, bool for_get, ViewPlan* out, std::string* err);

// The three views of tse_remap_view / tse_remap_view_plan -> out[0..2] = the plans of field, dp_src, dp_tgt.  Everything that needs no device:
// nf, the extent rules of a "qdp" get view with nf tracer slots and of two "dp" put views (remap_view_plan), and that the field's footprint
// meets neither grid's (remap_view_overlap, on the plans; tse_remap_view makes it after each footprint is known to lie in its allocation).
int remap_view_plan(int nelemd, int nf, const tse_view* field, const tse_view* dp_src, const tse_view* dp_tgt, ViewPlan out[3], std::string* err);
int remap_view_overlap(const tse_view* field, const tse_view* dp_src, const tse_view* dp_tgt, const ViewPlan plan[3], std::string* err);

// The view of tse_dss_view / tse_dss_view_plan: nf field slots of nk levels (1 <= nk <= NLEVP), the rules of a "qdp" get view except that an
// axis of extent 1 may carry stride 0.  lib[] are the strides of the staging field [e][f * nk + k][16]; path 1 only for nk == NLEV.
// who: the entry the refusals name.
int dss_view_plan(int nelemd, int nf, int nk, const tse_view* field, ViewPlan* out, std::string* err, const char* who = "tse_dss_view");

// The two views of tse_biharmonic_view / tse_biharmonic_view_plan -> out[0..1] = the plans of in, out: each a view of tse_dss_view.
// biharmonic_view_in_place: out is the same pointer and the same five strides as in.  biharmonic_view_overlap: otherwise the two
// footprints, each taken from its ptr, are disjoint (touching is disjoint).
// who: the entry the refusals name.
int biharmonic_view_plan(int nelemd, int nf, int nk, const tse_view* in, const tse_view* out_view, ViewPlan out[2], std::string* err,
                         const char* who = "tse_biharmonic_view");
bool biharmonic_view_in_place(const tse_view* in, const tse_view* out);
int biharmonic_view_overlap(const tse_view* in, const tse_view* out, const ViewPlan plan[2], std::string* err, const char* who = "tse_biharmonic_view");

// The two views of tse_vlaplace_view / tse_vlaplace_view_plan: those of tse_biharmonic_view with nf = 2 (the q axis is the wind component).
int vlaplace_view_plan(int nelemd, int nk, const tse_view* in, const tse_view* out_view, ViewPlan out[2], std::string* err);

// The two views of tse_sphere_op_view / tse_sphere_op_view_plan: each a view of tse_dss_view with its own field count, (nf_in, nf_out) =
// (1, 2) for TSE_OP_GRADIENT and (2, 1) for TSE_OP_DIVERGENCE and TSE_OP_VORTICITY (sphere_op_fields; false: no such op).  The shapes
// differ, so there is no in-place form: sphere_op_view_overlap asks for disjoint footprints (touching is disjoint).
bool sphere_op_fields(int op, int* nf_in, int* nf_out);
int sphere_op_view_plan(int nelemd, int nk, int op, const tse_view* in, const tse_view* out_view, ViewPlan out[2], std::string* err);
int sphere_op_view_overlap(const tse_view* in, const tse_view* out, const ViewPlan plan[2], std::string* err);

// The up to three read-only views of tse_stats_view / tse_stats_view_plan -> out[0..2] = the plans of field, ref, weight: each a view of
// tse_dss_view, field and ref with nf fields, weight with one (its q stride is not looked at).  ref and weight may be null: path -1 and an
// empty footprint.  No overlap rule: nothing is written through a view.
int stats_view_plan(int nelemd, int nf, int nk, const tse_view* field, const tse_view* ref, const tse_view* weight, ViewPlan out[3], std::string* err);

// The up to five views of tse_column_view / tse_column_view_plan -> out[0..4] = the plans of dp, p, a, b, out: each a view of tse_dss_view
// with one field of NLEV levels, except b of TSE_COL_PHI (the surface field: one level) and out of TSE_COL_PINT (NLEVP).  Which views an
// op needs, may take and refuses is the table of the header; an absent view: path -1 and an empty footprint.  column_view_overlap: the
// footprint of out (v[4]), taken from its ptr, meets that of no input.
int column_view_plan(int nelemd, int op, const tse_view* dp, const tse_view* p, const tse_view* a, const tse_view* b, const tse_view* out_view, ViewPlan out[5],
                     std::string* err);
int column_view_overlap(const tse_view* const v[5], const ViewPlan plan[5], std::string* err);

// The up to four views of tse_hypervis_view / tse_hypervis_view_plan -> out[0..3] = the plans of s, v, s_out, v_out: s and s_out views of
// tse_dss_view with nf fields, v and v_out with 2.  s is absent exactly when nf == 0, v may be absent (not both); the out views are both
// absent or given for exactly the inputs.  An absent view: path -1 and an empty footprint.  Also refused: nf above HYPERVIS_MAX_FIELDS
// (the factors travel as kernel arguments) and nelemd * (nf + 2) * nk >= 2^27.  hypervis_view_overlap: every two views that are given
// are disjoint -- their footprints do not meet, or they have the same element stride and their footprints within one element are
// disjoint and lie together inside one element stride (the members of one elem(:)).
constexpr int HYPERVIS_MAX_FIELDS = TSE_HYPERVIS_MAX_FIELDS;
int hypervis_view_plan(int nelemd, int nf, int nk, const tse_view* s, const tse_view* v, const tse_view* s_out, const tse_view* v_out, ViewPlan out[4],
                       std::string* err);
int hypervis_view_overlap(const tse_view* const x[4], const ViewPlan plan[4], std::string* err);

// the message of tse_last_error, for the C entries of this host C++ unit: a call of tse::fail (tse_ctx.h; defined in tse_api.hip)
int set_last_error(const char* msg);

}  // namespace tse
