// tse_views.cpp -- descriptor logic of the strided device views (tse_views.h), and tse_view_plan.  Plain host C++17: no HIP header,
// no device; tests/test_views_cpu.py holds it to a brute-force model (tests/view_model.py).
#include "tse_views.h"

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>

namespace tse {

namespace {

const char* const AXIS[5] = {"element", "q", "level", "j", "i"};

// qkind: 0 no q axis, 1 the tracers, 2 the two wind components.  Level extents of the view per direction (0: no level axis; -1: the
// field is not served in that direction).  liblev: levels per element of the library's array.
struct FieldDesc { const char* name; int field; int qkind; int lev_put, lev_get, liblev; };
const FieldDesc FIELDS[] = {
    {"qdp", VF_QDP, 1, NLEV, NLEV, NLEV},
    {"vn0", VF_VN0, 2, NLEV, -1, NLEV},
    {"dp", VF_DP, 0, NLEV, -1, NLEV},
    {"eta_dot_dpdn", VF_ETA, 0, NLEVP, NLEV, NLEVP},   // get: levels 1..nlev only, as tse_get_derived
    {"omega_p", VF_OMEGA_P, 0, NLEV, NLEV, NLEV},
    {"divdp", VF_DIVDP, 0, NLEV, NLEV, NLEV},
    {"divdp_proj", VF_DIVDP_PROJ, 0, NLEV, NLEV, NLEV},
    {"dp3d", VF_DP3D, 0, -1, NLEV, NLEV},
    {"ps_v", VF_PS_V, 0, -1, 0, 0},
    {"q", VF_Q, 1, -1, NLEV, NLEV},
    {"lnps", VF_LNPS, 0, -1, 0, 0},
};

int refuse(std::string* err, const char* fmt, ...) {
  char buf[384];
  va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
  if (err) *err = buf;
  return 1;
}

}  // namespace

// The part of a plan that follows the extents: the footprint, for a destination view that no two index tuples share an address, and the
// path the strides take.
static int footprint_and_path(const char* who, ViewPlan& p, const long long* s, bool for_get, bool has_level, std::string* err) {
  // footprint; every product in 128 bits, refused beyond 2^60 doubles
  const __int128 LIMIT = (__int128)1 << 60;
  __int128 lo = 0, hi = 0;
  for (int a = 0; a < 5; a++) {
    const __int128 span = (__int128)s[a] * (p.ext[a] - 1);
    if (span > LIMIT || span < -LIMIT) return refuse(err, "%s: the %s stride %lld is out of range", who, AXIS[a], s[a]);
    if (span < 0) lo += span; else hi += span;
  }
  p.lo = (long long)lo; p.hi = (long long)hi + 1;

  if (for_get) {
    // no two index tuples on one address: the axes that move (extent > 1) sorted by |stride|, each at least the previous one's stride
    // times its extent.  Sufficient, not necessary: an interleaved but disjoint view is refused too.
    int idx[5], n = 0;
    for (int a = 0; a < 5; a++) if (p.ext[a] > 1) idx[n++] = a;
    auto mag = [&](int a) { return s[a] < 0 ? -(__int128)s[a] : (__int128)s[a]; };
    std::stable_sort(idx, idx + n, [&](int x, int y) { return mag(x) < mag(y); });
    for (int i = 1; i < n; i++)
      if (mag(idx[i]) < mag(idx[i - 1]) * p.ext[idx[i - 1]])
        return refuse(err, "%s: the view may overlap itself: the %s stride (%lld) is smaller than the %s stride (%lld) times its extent %d", who,
                      AXIS[idx[i]], s[idx[i]], AXIS[idx[i - 1]], s[idx[i - 1]], p.ext[idx[i - 1]]);
  }

  const long long S = s[4];
  if (s[4] == 1 && s[3] == NP) p.path = 0;
  else if (has_level && s[2] == 1 && S >= p.ext[2] && s[3] == NP * S) p.path = 1;
  else p.path = 2;
  return 0;
}

bool view_wide(int path, const tse_view* v) {
  const long long* s = v->stride;
  if (path > 1 || ((uintptr_t)v->ptr & 15) || s[0] % 2 || s[1] % 2) return false;
  return s[path == 0 ? 2 : 4] % 2 == 0;
}

int view_plan(const char* field, int nelemd, int qsize, const tse_view* v, bool for_get, ViewPlan* out, std::string* err) {
  const char* who = for_get ? "tse_view_get" : "tse_view_put";
  if (!field || !v || !out) return refuse(err, "%s: null %s", who, !field ? "field name" : !v ? "view" : "plan");
  if (nelemd <= 0 || qsize <= 0) return refuse(err, "%s: nelemd = %d, qsize = %d", who, nelemd, qsize);
  const FieldDesc* f = nullptr;
  for (const FieldDesc& d : FIELDS) if (!strcmp(d.name, field)) f = &d;
  if (!f) return refuse(err, "%s: unknown field \"%s\"", who, field);
  const int lev = for_get ? f->lev_get : f->lev_put;
  if (lev < 0) return refuse(err, for_get ? "%s: field \"%s\" cannot be read through a view" : "%s: field \"%s\" cannot be written through a view", who, field);

  ViewPlan p;
  p.field = f->field;
  const bool has[5] = {true, f->qkind != 0, lev > 0, true, true};
  p.ext[0] = nelemd; p.ext[1] = f->qkind == 1 ? qsize : f->qkind == 2 ? 2 : 1; p.ext[2] = lev > 0 ? lev : 1; p.ext[3] = NP; p.ext[4] = NP;
  // the library's dense array: [e][q][k][16], vn0 [e][k][c][16], level fields [e][k][16], ps_v / lnps [e][16]
  const long long slab = NP * NP;
  p.lib[4] = 1; p.lib[3] = NP;
  if (f->qkind == 2) { p.lib[1] = slab; p.lib[2] = 2 * slab; p.lib[0] = 2 * slab * f->liblev; }
  else {
    p.lib[2] = has[2] ? slab : 0;
    p.lib[1] = has[1] ? slab * f->liblev : 0;
    p.lib[0] = slab * (has[2] ? f->liblev : 1) * (has[1] ? qsize : 1);
  }

  const long long* s = v->stride;
  for (int a = 0; a < 5; a++) {
    if (!has[a] && s[a] != 0) return refuse(err, "%s: field \"%s\" has no %s axis: its stride must be 0 (got %lld)", who, field, AXIS[a], s[a]);
    if (has[a] && for_get && s[a] == 0) return refuse(err, "%s: stride 0 on the %s axis: a destination view may not broadcast", who, AXIS[a]);
  }

  if (footprint_and_path(who, p, s, for_get, has[2], err)) return 1;
  *out = p;
  return 0;
}

// tse_remap_view's three views: `field` a "qdp" get view of nf tracer slots (written in place: no zero stride, no two index tuples on one
// address), dp_src and dp_tgt "dp" put views (a zero stride broadcasts).  remap_view_overlap: the field's footprint, taken from its ptr,
// may meet neither grid's -- the kernel reads the grids of an element while it writes the element's field.
int remap_view_plan(int nelemd, int nf, const tse_view* field, const tse_view* dp_src, const tse_view* dp_tgt, ViewPlan out[3], std::string* err) {
  const char* who = "tse_remap_view";
  if (!field || !dp_src || !dp_tgt || !out) return refuse(err, "%s: null view", who);
  if (nf < 1) return refuse(err, "%s: nf = %d (at least one field)", who, nf);
  const tse_view* v[3] = {field, dp_src, dp_tgt};
  const char* name[3] = {"field", "dp_src", "dp_tgt"};
  for (int i = 0; i < 3; i++) {
    std::string e;
    if (view_plan(i == 0 ? "qdp" : "dp", nelemd, nf, v[i], i == 0, &out[i], &e)) return refuse(err, "%s: %s: %s", who, name[i], e.c_str());
  }
  return 0;
}

int remap_view_overlap(const tse_view* field, const tse_view* dp_src, const tse_view* dp_tgt, const ViewPlan out[3], std::string* err) {
  const char* who = "tse_remap_view";
  const tse_view* v[3] = {field, dp_src, dp_tgt};
  const char* name[3] = {"field", "dp_src", "dp_tgt"};
  for (int i = 1; i < 3; i++) {
    if (Footprint(field, out[0]).meets(Footprint(v[i], out[i])))
      return refuse(err, "%s: the field [%p%+lld, %p%+lld doubles) overlaps %s [%p%+lld, %p%+lld doubles): it is remapped in place while the grids are read", who,
                    field->ptr, out[0].lo, field->ptr, out[0].hi, name[i], v[i]->ptr, out[i].lo, v[i]->ptr, out[i].hi);
  }
  return 0;
}

// tse_dss_view's view: the rules of a "qdp" get view (written in place) with nf field slots on the q axis and nk levels; an axis of extent
// 1 may carry any stride, 0 included.  The dense side is the staging field [e][f * nk + k][16].  Path 1 exists for nk == NLEV alone: a
// level-fastest view of another depth takes the generic path, and the plan says so.
int dss_view_plan(int nelemd, int nf, int nk, const tse_view* v, ViewPlan* out, std::string* err, const char* who) {
  if (!v || !out) return refuse(err, "%s: null %s", who, !v ? "view" : "plan");
  if (nelemd <= 0) return refuse(err, "%s: nelemd = %d", who, nelemd);
  if (nf < 1) return refuse(err, "%s: nf = %d (at least one field)", who, nf);
  if (nk < 1 || nk > NLEVP) return refuse(err, "%s: nk = %d (1 to nlev + 1 = %d levels)", who, nk, NLEVP);
  if ((long long)nf * nk >= (1ll << 24)) return refuse(err, "%s: nf * nk = %lld layers", who, (long long)nf * nk);
  ViewPlan p;
  p.field = VF_QDP;
  p.ext[0] = nelemd; p.ext[1] = nf; p.ext[2] = nk; p.ext[3] = NP; p.ext[4] = NP;
  const long long slab = NP * NP;
  p.lib[4] = 1; p.lib[3] = NP; p.lib[2] = slab; p.lib[1] = slab * nk; p.lib[0] = slab * nk * nf;
  const long long* s = v->stride;
  for (int a = 0; a < 5; a++)
    if (p.ext[a] > 1 && s[a] == 0) return refuse(err, "%s: stride 0 on the %s axis (extent %d): the field is written in place and may not broadcast", who, AXIS[a], p.ext[a]);
  if (footprint_and_path(who, p, s, true, true, err)) return 1;
  if (p.path == 1 && nk != NLEV) p.path = 2;
  *out = p;
  return 0;
}

// tse_biharmonic_view's two views: each a view of tse_dss_view (dss_view_plan).  biharmonic_view_overlap: `out` is `in` itself (the same
// pointer and the same five strides: in place) or its footprint, taken from its ptr, does not meet in's -- the first kernel reads `in`
// whole before the second writes `out`, but a partial overlap would leave a field that is neither the input nor the result.
int biharmonic_view_plan(int nelemd, int nf, int nk, const tse_view* in, const tse_view* out_view, ViewPlan out[2], std::string* err, const char* who) {
  if (!in || !out_view || !out) return refuse(err, "%s: null view", who);
  const tse_view* v[2] = {in, out_view};
  for (int i = 0; i < 2; i++) {
    std::string e;
    if (dss_view_plan(nelemd, nf, nk, v[i], &out[i], &e, who)) return refuse(err, "%s (%s)", e.c_str(), i == 0 ? "in" : "out");
  }
  return 0;
}

bool biharmonic_view_in_place(const tse_view* in, const tse_view* out) {
  if (in->ptr != out->ptr) return false;
  for (int a = 0; a < 5; a++) if (in->stride[a] != out->stride[a]) return false;
  return true;
}

int biharmonic_view_overlap(const tse_view* in, const tse_view* out, const ViewPlan plan[2], std::string* err, const char* who) {
  if (biharmonic_view_in_place(in, out)) return 0;
  if (Footprint(in, plan[0]).meets(Footprint(out, plan[1])))
    return refuse(err, "%s: out [%p%+lld, %p%+lld doubles) overlaps in [%p%+lld, %p%+lld doubles) without being the same view (the same "
                  "pointer and strides: in place)", who, out->ptr, plan[1].lo, out->ptr, plan[1].hi, in->ptr, plan[0].lo, in->ptr, plan[0].hi);
  return 0;
}

// tse_vlaplace_view's two views: each a view of tse_dss_view with nf = 2, the q axis the wind component; the overlap rule is
// biharmonic_view_overlap's.
int vlaplace_view_plan(int nelemd, int nk, const tse_view* in, const tse_view* out_view, ViewPlan out[2], std::string* err) {
  return biharmonic_view_plan(nelemd, 2, nk, in, out_view, out, err, "tse_vlaplace_view");
}

// tse_sphere_op_view's two views: each a view of tse_dss_view, `in` with nf_in fields and `out` with nf_out.
bool sphere_op_fields(int op, int* nf_in, int* nf_out) {
  if (op < TSE_OP_GRADIENT || op > TSE_OP_VORTICITY) return false;
  *nf_in = op == TSE_OP_GRADIENT ? 1 : 2;
  *nf_out = op == TSE_OP_GRADIENT ? 2 : 1;
  return true;
}

int sphere_op_view_plan(int nelemd, int nk, int op, const tse_view* in, const tse_view* out_view, ViewPlan out[2], std::string* err) {
  const char* who = "tse_sphere_op_view";
  int nf[2];
  if (!sphere_op_fields(op, &nf[0], &nf[1])) return refuse(err, "%s: op=%d (0: gradient_sphere, 1: divergence_sphere, 2: vorticity_sphere)", who, op);
  if (!in || !out_view || !out) return refuse(err, "%s: null view", who);
  const tse_view* v[2] = {in, out_view};
  for (int i = 0; i < 2; i++) {
    std::string e;
    if (dss_view_plan(nelemd, nf[i], nk, v[i], &out[i], &e, who)) return refuse(err, "%s (%s)", e.c_str(), i == 0 ? "in" : "out");
  }
  return 0;
}

int sphere_op_view_overlap(const tse_view* in, const tse_view* out, const ViewPlan plan[2], std::string* err) {
  if (Footprint(in, plan[0]).meets(Footprint(out, plan[1])))
    return refuse(err, "tse_sphere_op_view: out [%p%+lld, %p%+lld doubles) overlaps in [%p%+lld, %p%+lld doubles): the shapes differ, there is no in-place form",
                  out->ptr, plan[1].lo, out->ptr, plan[1].hi, in->ptr, plan[0].lo, in->ptr, plan[0].hi);
  return 0;
}

// tse_stats_view's up to three views, all read-only: `field` and `ref` views of tse_dss_view with nf fields of nk levels, `weight` one
// with a single field whose q stride is not looked at (every field reads the same weight).  An absent view (null) leaves path -1 and an
// empty footprint.  The views may overlap each other.
int stats_view_plan(int nelemd, int nf, int nk, const tse_view* field, const tse_view* ref, const tse_view* weight, ViewPlan out[3], std::string* err) {
  const char* who = "tse_stats_view";
  if (!field || !out) return refuse(err, "%s: null %s", who, !field ? "view" : "plan");
  const tse_view* v[3] = {field, ref, weight};
  const char* role[3] = {"field", "ref", "weight"};
  for (int i = 0; i < 3; i++) {
    out[i] = ViewPlan();
    out[i].path = -1;
    if (!v[i]) continue;
    std::string e;
    if (dss_view_plan(nelemd, i == 2 ? 1 : nf, nk, v[i], &out[i], &e, who)) return refuse(err, "%s (%s)", e.c_str(), role[i]);
  }
  return 0;
}

// tse_column_view's up to five views -- dp, p, a, b, out -- each a view of tse_dss_view with one field: which of them the op needs, may
// take or refuses (the table of the header), and the level count of each: NLEV, 1 for the surface view b of PHI (whose level stride is
// not looked at), NLEVP for the out of PINT.  An absent view leaves path -1 and an empty footprint.
static const char* const COLUMN_ROLE[5] = {"dp", "p", "a", "b", "out"};

int column_view_plan(int nelemd, int op, const tse_view* dp, const tse_view* p, const tse_view* a, const tse_view* b, const tse_view* out_view, ViewPlan out[5],
                     std::string* err) {
  const char* who = "tse_column_view";
  if (op < TSE_COL_PINT || op > TSE_COL_OMEGA)
    return refuse(err, "%s: op=%d (0: interface pressure, 1: mid-point pressure, 2: geopotential, 3: omega / p)", who, op);
  if (!out) return refuse(err, "%s: null plan", who);
  const tse_view* v[5] = {dp, p, a, b, out_view};
  // 1 needed, 0 must be null, 2 optional
  const bool scan = op <= TSE_COL_PMID;
  const int want[5] = {op == TSE_COL_OMEGA ? (p ? 0 : 1) : 1, scan ? 0 : 2, scan ? 0 : 1, scan ? 0 : 1, 1};
  static const char* const opname[4] = {"TSE_COL_PINT", "TSE_COL_PMID", "TSE_COL_PHI", "TSE_COL_OMEGA"};
  for (int i = 0; i < 5; i++) {
    if (want[i] == 1 && !v[i]) return refuse(err, "%s: %s needs the view %s%s", who, opname[op], COLUMN_ROLE[i], op == TSE_COL_OMEGA && i == 0 ? " when p is null" : "");
    if (want[i] == 0 && v[i]) return refuse(err, "%s: %s takes no view %s%s: pass null", who, opname[op], COLUMN_ROLE[i], op == TSE_COL_OMEGA && i == 0 ? " beside p" : "");
  }
  for (int i = 0; i < 5; i++) {
    out[i] = ViewPlan();
    out[i].path = -1;
    if (!v[i]) continue;
    const int nk = i == 4 && op == TSE_COL_PINT ? NLEVP : i == 3 && op == TSE_COL_PHI ? 1 : NLEV;
    std::string e;
    if (dss_view_plan(nelemd, 1, nk, v[i], &out[i], &e, who)) return refuse(err, "%s (%s)", e.c_str(), COLUMN_ROLE[i]);
  }
  return 0;
}

int column_view_overlap(const tse_view* const v[5], const ViewPlan plan[5], std::string* err) {
  for (int i = 0; i < 4; i++) {
    if (!v[i]) continue;
    if (Footprint(v[i], plan[i]).meets(Footprint(v[4], plan[4])))
      return refuse(err, "tse_column_view: out [%p%+lld, %p%+lld doubles) overlaps %s [%p%+lld, %p%+lld doubles): a column is read while it is written", v[4]->ptr,
                    plan[4].lo, v[4]->ptr, plan[4].hi, COLUMN_ROLE[i], v[i]->ptr, plan[i].lo, v[i]->ptr, plan[i].hi);
  }
  return 0;
}

// tse_hypervis_view's up to four views -- s, v, s_out, v_out: s and s_out views of tse_dss_view with nf fields, v and v_out with 2 (the q
// axis is the wind component).  s is absent exactly when nf == 0, v may be absent, not both; the out views are both absent (the update is
// in place) or given for exactly the inputs that are present.  An absent view leaves path -1 and an empty footprint.
static const char* const HYPERVIS_ROLE[4] = {"s", "v", "s_out", "v_out"};

int hypervis_view_plan(int nelemd, int nf, int nk, const tse_view* s, const tse_view* v, const tse_view* s_out, const tse_view* v_out, ViewPlan out[4],
                       std::string* err) {
  const char* who = "tse_hypervis_view";
  if (!out) return refuse(err, "%s: null plan", who);
  if (nf < 0) return refuse(err, "%s: nf = %d (the number of scalar fields: 0 or more)", who, nf);
  if (nf > HYPERVIS_MAX_FIELDS) return refuse(err, "%s: nf = %d (at most %d scalar fields in one call: their factors travel as kernel arguments)", who, nf, HYPERVIS_MAX_FIELDS);
  if ((nf == 0) != (s == nullptr)) return refuse(err, nf ? "%s: nf = %d needs the view s" : "%s: nf = %d takes no view s: pass null", who, nf);
  if (!s && !v) return refuse(err, "%s: neither scalar fields (nf = 0, s null) nor a wind (v null): nothing to do", who);
  const tse_view* x[4] = {s, v, s_out, v_out};
  if (s_out || v_out)
    for (int i = 0; i < 2; i++) {
      if (x[i] && !x[i + 2]) return refuse(err, "%s: %s is given and %s is not: the out views are both null (in place) or given for exactly the inputs", who, HYPERVIS_ROLE[i], HYPERVIS_ROLE[i + 2]);
      if (!x[i] && x[i + 2]) return refuse(err, "%s: %s is given and %s is not: an out view belongs to an input", who, HYPERVIS_ROLE[i + 2], HYPERVIS_ROLE[i]);
    }
  for (int i = 0; i < 4; i++) {
    out[i] = ViewPlan();
    out[i].path = -1;
    if (!x[i]) continue;
    std::string e;
    if (dss_view_plan(nelemd, i & 1 ? 2 : nf, nk, x[i], &out[i], &e, who)) return refuse(err, "%s (%s)", e.c_str(), HYPERVIS_ROLE[i]);
  }
  const long long nl = (long long)(nf + (v ? 2 : 0)) * nk;
  if ((long long)nelemd * nl >= (1ll << 27)) return refuse(err, "%s: %d elements x %lld layers (the launches count 32-bit blocks)", who, nelemd, nl);
  return 0;
}

// Whether two views may share an address.  Not when their footprints, each taken from its ptr, are disjoint (touching is disjoint).  Two
// members of one elem(:) -- T, dp3d and state%v of E3SM -- interleave, so their footprints meet although no address is shared: two views
// of the same element stride are also disjoint when their footprints within ONE element (the axes q, level, j, i) are disjoint and lie
// together inside one element stride -- element e of one and element e' of the other then sit in windows a whole stride apart.
static bool views_may_meet(const tse_view* a, const ViewPlan& pa, const tse_view* b, const ViewPlan& pb) {
  if (!Footprint(a, pa).meets(Footprint(b, pb))) return false;
  const __int128 es = a->stride[0] < 0 ? -(__int128)a->stride[0] : (__int128)a->stride[0];
  if (a->stride[0] != b->stride[0] || es == 0 || pa.ext[0] != pb.ext[0]) return true;
  __int128 lo[2], hi[2];
  const tse_view* v[2] = {a, b};
  const ViewPlan* p[2] = {&pa, &pb};
  for (int i = 0; i < 2; i++) {
    lo[i] = hi[i] = (__int128)(uintptr_t)v[i]->ptr;
    for (int ax = 1; ax < 5; ax++) {
      const __int128 span = (__int128)v[i]->stride[ax] * (p[i]->ext[ax] - 1) * 8;
      if (span < 0) lo[i] += span; else hi[i] += span;
    }
    hi[i] += 8;
  }
  if (lo[0] < hi[1] && lo[1] < hi[0]) return true;
  return std::max(hi[0], hi[1]) - std::min(lo[0], lo[1]) > es * 8;
}

// Every pair of the views that are given is disjoint (views_may_meet): in place both s and v are written, and an out view is written
// while both inputs are still read.
int hypervis_view_overlap(const tse_view* const x[4], const ViewPlan plan[4], std::string* err) {
  for (int i = 0; i < 4; i++)
    for (int j = i + 1; j < 4; j++) {
      if (!x[i] || !x[j]) continue;
      if (views_may_meet(x[i], plan[i], x[j], plan[j]))
        return refuse(err, "tse_hypervis_view: %s [%p%+lld, %p%+lld doubles) overlaps %s [%p%+lld, %p%+lld doubles): the views of one call are disjoint",
                      HYPERVIS_ROLE[j], x[j]->ptr, plan[j].lo, x[j]->ptr, plan[j].hi, HYPERVIS_ROLE[i], x[i]->ptr, plan[i].lo, x[i]->ptr, plan[i].hi);
    }
  return 0;
}

}  // namespace tse

// the C plan entries: an error becomes the message of tse_last_error; n plans go out as path[] / lo[] / hi[], each of them optional
static int refused(const std::string& err) { return tse::set_last_error(err.c_str()); }
static int plans_out(const tse::ViewPlan* p, int n, int* path, long long* lo, long long* hi) {
  for (int i = 0; i < n; i++) {
    if (path) path[i] = p[i].path;
    if (lo) lo[i] = p[i].lo;
    if (hi) hi[i] = p[i].hi;
  }
  return 0;
}

extern "C" int tse_view_plan(const char* field, int nelemd, int qsize, const tse_view* v, int for_get, int* path, long long* lo, long long* hi) {
  tse::ViewPlan p;
  std::string err;
  if (tse::view_plan(field, nelemd, qsize, v, for_get != 0, &p, &err)) return refused(err);
  return plans_out(&p, 1, path, lo, hi);
}

extern "C" int tse_remap_view_plan(int nelemd, int nf, const tse_view* field, const tse_view* dp_src, const tse_view* dp_tgt, int path[3], long long lo[3],
                                   long long hi[3]) {
  tse::ViewPlan p[3];
  std::string err;
  if (tse::remap_view_plan(nelemd, nf, field, dp_src, dp_tgt, p, &err)) return refused(err);
  // strides alone (all three ptr null): nothing is known of where the views lie
  if ((field->ptr || dp_src->ptr || dp_tgt->ptr) && tse::remap_view_overlap(field, dp_src, dp_tgt, p, &err)) return refused(err);
  return plans_out(p, 3, path, lo, hi);
}

extern "C" int tse_dss_view_plan(int nelemd, int nf, int nk, const tse_view* field, int* path, long long* lo, long long* hi) {
  tse::ViewPlan p;
  std::string err;
  if (tse::dss_view_plan(nelemd, nf, nk, field, &p, &err)) return refused(err);
  return plans_out(&p, 1, path, lo, hi);
}

extern "C" int tse_biharmonic_view_plan(int nelemd, int nf, int nk, const tse_view* in, const tse_view* out, int path[2], long long lo[2], long long hi[2]) {
  tse::ViewPlan p[2];
  std::string err;
  if (tse::biharmonic_view_plan(nelemd, nf, nk, in, out, p, &err)) return refused(err);
  // strides alone (both ptr null): nothing is known of where the views lie
  if ((in->ptr || out->ptr) && tse::biharmonic_view_overlap(in, out, p, &err)) return refused(err);
  return plans_out(p, 2, path, lo, hi);
}

extern "C" int tse_vlaplace_view_plan(int nelemd, int nk, const tse_view* in, const tse_view* out, int path[2], long long lo[2], long long hi[2]) {
  tse::ViewPlan p[2];
  std::string err;
  if (tse::vlaplace_view_plan(nelemd, nk, in, out, p, &err)) return refused(err);
  // strides alone (both ptr null): nothing is known of where the views lie
  if ((in->ptr || out->ptr) && tse::biharmonic_view_overlap(in, out, p, &err, "tse_vlaplace_view")) return refused(err);
  return plans_out(p, 2, path, lo, hi);
}

extern "C" int tse_sphere_op_view_plan(int nelemd, int nk, int op, const tse_view* in, const tse_view* out, int path[2], long long lo[2], long long hi[2]) {
  tse::ViewPlan p[2];
  std::string err;
  if (tse::sphere_op_view_plan(nelemd, nk, op, in, out, p, &err)) return refused(err);
  // strides alone (both ptr null): nothing is known of where the views lie
  if ((in->ptr || out->ptr) && tse::sphere_op_view_overlap(in, out, p, &err)) return refused(err);
  return plans_out(p, 2, path, lo, hi);
}

extern "C" int tse_stats_view_plan(int nelemd, int nf, int nk, const tse_view* field, const tse_view* ref, const tse_view* weight, int path[3], long long lo[3],
                                   long long hi[3]) {
  tse::ViewPlan p[3];
  std::string err;
  if (tse::stats_view_plan(nelemd, nf, nk, field, ref, weight, p, &err)) return refused(err);
  return plans_out(p, 3, path, lo, hi);
}

extern "C" int tse_column_view_plan(int nelemd, int op, const tse_view* dp, const tse_view* p, const tse_view* a, const tse_view* b, const tse_view* out,
                                    int path[5], long long lo[5], long long hi[5]) {
  tse::ViewPlan pl[5];
  std::string err;
  if (tse::column_view_plan(nelemd, op, dp, p, a, b, out, pl, &err)) return refused(err);
  // strides alone (every ptr null): nothing is known of where the views lie
  const tse_view* v[5] = {dp, p, a, b, out};
  bool placed = false;
  for (const tse_view* x : v) placed = placed || (x && x->ptr);
  if (placed && tse::column_view_overlap(v, pl, &err)) return refused(err);
  return plans_out(pl, 5, path, lo, hi);
}

extern "C" int tse_hypervis_view_plan(int nelemd, int nf, int nk, const tse_view* s, const tse_view* v, const tse_view* s_out, const tse_view* v_out, int path[4],
                                      long long lo[4], long long hi[4]) {
  tse::ViewPlan p[4];
  std::string err;
  if (tse::hypervis_view_plan(nelemd, nf, nk, s, v, s_out, v_out, p, &err)) return refused(err);
  // strides alone (every ptr null): nothing is known of where the views lie
  const tse_view* x[4] = {s, v, s_out, v_out};
  bool placed = false;
  for (const tse_view* y : x) placed = placed || (y && y->ptr);
  if (placed && tse::hypervis_view_overlap(x, p, &err)) return refused(err);
  return plans_out(p, 4, path, lo, hi);
}

#ifdef TSE_AB_HOOKS
// view_wide for the CPU test that holds it to the addresses the kernels touch (tests/test_views_cpu.py); not in the product library
extern "C" int tse_test_view_wide(int path, const tse_view* v) { return tse::view_wide(path, v) ? 1 : 0; }
#endif
