// libtsl_hip.so -- C ABI (include/tsl_hip.h) over the gfx950 kernels.  Host orchestration of
//   BaseScene.compute_energy / compute_residual_and_Hessian / newton_step / time_step
//   (/root/reference/code/engine/BaseScene.py:427-451, :976-1040, :1159-1230, :1327-1370),
//   and SparseMatrix.solve (sparse_solver.py:85-105).  No kernel is defined here: device code lives in the k_*.hpp headers (k_scene.hpp: energy and
//   gradient gathers, k_adjoint.hpp: the reverse step), and the entry points of a subject in its own header, included below where what they call is
//   defined: handle_api.hpp (soft handles), param_api.hpp (read-outs of system identification; its key table and partial layout are host logic in
//   param_keys.hpp), adjoint_api.hpp (Grad.transfer_grad, analytic_grad_single.py:217-257), direct_host.hpp / direct_group.hpp (sparse direct solve),
//   mg_test_api.hpp (views of the iterative hierarchy and its parts run alone, for the tests).
// There is no CPU fallback in this library: without a HIP device every entry point fails.
#include <stdarg.h>
#include <cctype>
#include <chrono>
#include <mutex>

#include <array>
#include <map>

#include "k_cloth.hpp"
#include "k_contact.hpp"
#include "k_fem.hpp"
#include "k_mg.hpp"
#include "k_param.hpp"
#include "k_solver.hpp"
#include "param_keys.hpp"
#include "tsl_ctx.hpp"

thread_local std::string g_tsl_err;
int tsl_fail(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_tsl_err = buf;
  return -1;
}

#define TSL_TRY(x) do { if ((x) != 0) return -1; } while (0)
#include "direct_host.hpp"
#include "direct_group.hpp"

#ifndef PCG_WPS
#define PCG_WPS 4
#endif
// matrix values: plain (temporal) loads -- the three operator products of a multigrid-PCG iteration re-read the same 41 MB,
// which stay in the 256 MB Infinity Cache; nontemporal loads were 2 % slower here (they won for the one-product block-Jacobi loop)
#ifndef TSL_NT
#define TSL_NT false
#endif
// partial sums + tickets of the deterministic dot products (k_dot / k_multi_dot; allocated at context creation, ticket rows start at zero)
#define DOT_SCRATCH(c) (c)->dot_part.p, (c)->dot_ticket.p
#define DOT_BLOCKS 120  // one f64 atomic per wave into a single address: more blocks only add contention (30 us at 600 blocks)
static inline int nblk(long n, int b) { return (int)((n + b - 1) / b); }
static inline int gsz(size_t n) { size_t b = (n + 255) / 256; return (int)std::min<size_t>(std::max<size_t>(b, 1), 4096); }
#include "handle_api.hpp"
#include "tie_api.hpp"
#include "collider_api.hpp"
#include "wind_api.hpp"
#include "k_scene.hpp"

// ------------------------------------------------------------------------------------------------
static int mg_build(tsl_ctx* c, const tsl_scene_desc* d);
static int body_dense_setup(tsl_ctx* c);
static bool body_active(tsl_ctx* c);
static void body_zero_dinv(tsl_ctx* c);
static bool direct_takes_solve(tsl_ctx* c);
static int block_jacobi_refresh(tsl_ctx* c);
extern "C" const char* tsl_version(void) { return "tsl-hip 0.1 gfx950 fp64"; }
extern "C" const char* tsl_last_error(void) { return g_tsl_err.c_str(); }

static ClothArgs cloth_args(tsl_ctx* c) {
  ClothArgs A;
  A.n_cface = c->n_cface; A.n_hinge = c->n_hinge; A.cloth = c->d_cloth.p;
  A.f2v = c->cf_f2v.p; A.cf = c->cf_cf.p; A.cp = c->cf_cp.p; A.cid = c->cf_cloth.p;
  A.V = c->cf_V.p; A.li = c->cf_li.p; A.hg_info = c->hg_info.p; A.hg_v = c->hg_v.p; A.norm_dir = c->norm_dir.p; A.f_order = c->cf_order.p;
  A.gstage = nullptr; A.gs_hinge = c->vg_hinge0;
  return A;
}
static StvkArgs stvk_args(tsl_ctx* c) { return StvkArgs{c->d_stvk.p, c->cf_dminv.p}; }
static VertArgs vert_args(tsl_ctx* c) {
  VertArgs A;
  A.NV = c->NV; A.mass = c->mass.p; A.grav = c->grav.p; A.fext = c->fext.p; A.dt = c->dt;
  return A;
}
static TetArgs tet_args(tsl_ctx* c) {
  TetArgs A;
  A.n_tet = c->n_tet; A.el = c->d_el.p; A.tv = c->tet_v.p; A.tel = c->tet_el.p; A.B = c->tet_B.p; A.W = c->tet_W.p; A.gstage = nullptr;
  return A;
}
static ContactArgs contact_args(tsl_ctx* c) {
  ContactArgs A;
  A.idx = c->c_idx.p; A.w = c->c_w.p; A.n = c->c_n.p; A.dx0 = c->c_dx0.p; A.k = c->c_k.p; A.mu = c->c_mu.p; A.T = c->c_T.p;
  A.k_contact = c->k_contact; A.eps_contact = c->eps_contact; A.eps_vh = c->eps_v * c->dt;
  return A;
}

static int upload_frozen(tsl_ctx* c) {
  TSL_TRY(c->frozen.upload(c->h_frozen));
  std::vector<unsigned char> fz(c->NV);
  std::vector<double> md(c->NV);
  for (int p = 0; p < c->NV; p++) {
    const int v = c->h_perm[p];
    fz[p] = (unsigned char)((c->h_frozen[3 * v] ? 1 : 0) | (c->h_frozen[3 * v + 1] ? 2 : 0) | (c->h_frozen[3 * v + 2] ? 4 : 0));
    md[p] = c->h_mass[v] / (c->dt * c->dt);
  }
  TSL_TRY(c->fzmask.upload(fz));
  TSL_TRY(c->mdt2.upload(md));
  return 0;
}

extern "C" int tsl_ctx_create(const tsl_scene_desc* d, tsl_ctx** out) {
  if (!d || !out) return tsl_fail("tsl_ctx_create: null argument");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return tsl_fail("tsl_ctx_create: no HIP device (this engine has no CPU path)");
  std::unique_ptr<tsl_ctx> owner(new tsl_ctx());   // every failure exit below releases what exists by then (~tsl_ctx)
  tsl_ctx* c = owner.get();
  const auto no_stream = [](hipStream_t* s) { return hipStreamCreateWithFlags(s, hipStreamNonBlocking) != hipSuccess; };
  const auto no_event = [](hipEvent_t* e) { return hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess; };
  if (no_stream(&c->stream) || no_event(&c->ev_in) || no_event(&c->ev_out)) return tsl_fail("stream / event creation failed");
  c->NV = d->tot_NV; c->NF = d->tot_NF;
  if (d->tot_NF > 0 && d->faces_host) c->h_faces.assign(d->faces_host, d->faces_host + 3 * (size_t)d->tot_NF);
  c->dt = d->dt; c->k_contact = d->k_contact; c->eps_contact = d->eps_contact; c->eps_v = d->eps_v; c->damping = d->damping;
  c->max_n_constraints = d->max_n_constraints > 0 ? d->max_n_constraints : 10000;
  c->grid_h = d->grid_h > 0 ? d->grid_h : 0.003;
  const int NV = c->NV;

  // ---- host tables (scene_tables.hpp): the counts and the copies the context keeps
  SceneTables T;
  std::string err;
  if (build_scene_tables(d, T, err)) return tsl_fail("%s", err.c_str());
  const Pattern& P = T.P;
  c->h_cloth = T.h_cloth; c->h_el = T.h_el; c->ds.grids = T.grids; c->ds.blocks = T.blocks;
  c->n_cface = T.n_cface; c->n_hinge = T.n_hinge; c->n_tet = T.n_tet;
  c->h_cf_f2v = T.f2v; c->h_cf_cf = T.cf; c->h_cf_cp = T.cp;
  c->h_rows = P.rows; c->h_perm = P.perm; c->h_rowpos = P.rowpos; c->h_slice_off = P.slice_off; c->h_slice_len = P.slice_len; c->h_colidx = P.colidx;
  c->n_slices = P.n_slices; c->n_slots = P.n_slots; c->nnzb = T.nnzb;
  c->n_cgblk = T.n_cgblk; c->n_cgblk_cloth = T.n_cgblk_cloth;
  c->vg_hinge0 = T.vg_hinge0; c->vg_tet0 = T.vg_tet0; c->vg_ns = T.vg_ns;
  c->h_mass.assign(d->mass_host, d->mass_host + NV);
  c->h_frozen.assign(d->frozen_host, d->frozen_host + 3 * (size_t)NV);
  const std::vector<double> grav(d->gravity_host, d->gravity_host + 3 * (size_t)NV), fext(3 * (size_t)NV, 0.0);

  // ---- uploads (a failed one has set the error)
  if (c->d_cloth.upload(c->h_cloth) || c->cf_f2v.upload(T.f2v) || c->cf_cf.upload(T.cf) || c->cf_cp.upload(T.cp) || c->cf_cloth.upload(T.cid) || c->cf_V.upload(T.V) ||
      c->cf_li.upload(T.li) || c->cf_order.upload(T.forder) || c->cf_blk.upload(T.cfblk) || c->hg_info.upload(T.hinfo) || c->hg_v.upload(T.hv) || c->hg_blk.upload(T.hgblk)) return -1;
  if (c->n_cgblk > 0 && (c->cg_base.upload(T.cg_base) || c->cg_ptr.upload(T.cg_ptr) || c->cg_ent.upload(T.cg_ent))) return -1;
  if (c->vg_ptr.upload(T.vg_ptr) || (!T.vg_idx.empty() && c->vg_idx.upload(T.vg_idx)) || c->trans.upload(T.trans)) return -1;
  if (c->d_el.upload(c->h_el) || c->tet_v.upload(T.tv) || c->tet_el.upload(T.tel) || c->tet_blk.upload(T.tetblk) || c->tet_B.upload(T.tB) || c->tet_W.upload(T.tW)) return -1;
  if (c->diag_blk.upload(T.dblk) || c->rowpos.upload(P.rowpos) || c->perm.upload(P.perm) || c->slice_off.upload(P.slice_off) || c->slice_len.upload(P.slice_len) ||
      c->colidx.upload(P.colidx) || c->diag_perm.upload(P.diag_perm)) return -1;
  if (c->mass.upload(c->h_mass) || c->grav.upload(grav) || c->fext.upload(fext) || upload_frozen(c)) return -1;

  // ---- allocations
  int rc = 0;
  rc |= c->norm_dir.alloc((size_t)std::max(c->n_cface, 1) * 3);
  // (the element records of the gather assembly -- 81 doubles per face, 65 MB at 100k triangles -- are allocated at the first deterministic assembly)
  rc |= c->quirk.alloc((size_t)std::max(d->n_cloth, 1) * 90);
  rc |= c->dot_part.alloc(64 * 512); rc |= c->dot_ticket.alloc(512);
  if (!rc) (void)hipMemset(c->dot_ticket.p, 0, 512 * sizeof(int));
  rc |= c->vals.alloc((size_t)P.n_slots * 9); rc |= c->vals_full.alloc((size_t)P.n_slots * 9);
  rc |= c->Dinv.alloc((size_t)NV * 9);
  const size_t n3 = (size_t)NV * 3;
  rc |= c->v_x.alloc(n3); rc |= c->v_r.alloc(n3); rc |= c->v_z.alloc(n3); rc |= c->v_p.alloc(n3); rc |= c->v_Ap.alloc(n3); rc |= c->v_b.alloc(n3);
  rc |= c->v_t0.alloc(n3); rc |= c->v_t1.alloc(n3); rc |= c->v_t2.alloc(n3); rc |= c->v_t3.alloc(n3); rc |= c->v_t4.alloc(n3); rc |= c->v_mg.alloc(n3);
  rc |= c->F.alloc(n3); rc |= c->pdir.alloc(n3); rc |= c->x1.alloc(n3);
  rc |= c->scal.alloc(1);
  rc |= c->part_pAp.alloc((size_t)P.n_slices + (size_t)(c->max_n_constraints + 63) / 64 + 8); rc |= c->part_rz.alloc((size_t)NV / 256 + 8 + 1024); rc |= c->part_rr.alloc((size_t)NV / 256 + 8 + 1024);
  if (rc) return -1;
  if (hipHostMalloc((void**)&c->h_scal, sizeof(SolverScalars) > sizeof(CgScal) ? sizeof(SolverScalars) : sizeof(CgScal)) != hipSuccess ||
      hipHostMalloc((void**)&c->h_scal2, 2 * sizeof(SolverScalars)) != hipSuccess) return tsl_fail("hipHostMalloc failed");
  if (no_event(&c->rb_event[0]) || no_event(&c->rb_event[1])) return tsl_fail("hipEventCreate failed");
  if (no_stream(&c->side) || no_stream(&c->side2) || no_event(&c->ev_join2) || no_event(&c->ev_fork) || no_event(&c->ev_fork0) || no_event(&c->ev_g2) || no_event(&c->ev_hh) ||
      no_event(&c->ev_gf) || no_event(&c->ev_join)) return tsl_fail("side stream / event creation failed");
  c->vals.zero(); c->vals_full.zero(); c->scal.zero(); c->part_rz.zero(); c->part_rr.zero();

  // ---- contact tables, multigrid hierarchy, dense body blocks
  c->n_body = d->n_body; c->n_pair = d->n_pair;
  if (d->n_body > 0) c->h_bodies.assign(d->bodies, d->bodies + d->n_body);
  if (d->n_pair > 0) c->h_pairs.assign(d->pairs, d->pairs + d->n_pair);
  if (contact_alloc(c, d) || mg_build(c, d) || body_dense_setup(c)) return -1;
  (void)hipDeviceSynchronize();
  (void)hipGetDevice(&c->ds.device);
  *out = owner.release();
  return 0;
}

static void group_unregister_and_destroy(tsl_group* G);
extern "C" void tsl_ctx_destroy(tsl_ctx* c) {
  if (!c) return;
  if (c->group) group_unregister_and_destroy(c->group);   // (a member that goes takes the group with it: the others get buffers of their own again)
  (void)hipDeviceSynchronize();
  ds_flow_token_release(c->ds);   // (after the last launch of the context has ended)
  delete c;   // (~tsl_ctx, ~DirectSolver: whatever the context owns)
}

extern "C" int tsl_set_stream(tsl_ctx* c, void* s) { c->user_stream = (hipStream_t)s; return 0; }

// Dm^-1 of every cloth face for the StVK membrane, from the rest lengths l0 = |x0 - x1|, l1 = |x1 - x2|, l2 = |x2 - x0|: the rest triangle
// X0 = (0, 0), X1 = (l0, 0), X2 = (a, b), a = (l0^2 + l2^2 - l1^2) / (2 l0), b = sqrt(l2^2 - a^2); Dm = [X1 - X0, X2 - X0].  Built once.
static int stvk_prepare(tsl_ctx* c) {
  if (c->cf_dminv.n > 0 || c->n_cface == 0) return 0;
  std::vector<double> li(3 * (size_t)c->n_cface), dm(4 * (size_t)c->n_cface);
  HIP_OK(hipMemcpy(li.data(), c->cf_li.p, li.size() * sizeof(double), hipMemcpyDeviceToHost));
  std::vector<int> cid(c->n_cface);
  HIP_OK(hipMemcpy(cid.data(), c->cf_cloth.p, cid.size() * sizeof(int), hipMemcpyDeviceToHost));
  for (int f = 0; f < c->n_cface; f++) {
    const double l0 = li[3 * f], l1 = li[3 * f + 1], l2 = li[3 * f + 2];
    if (!(l0 > 0 && l1 > 0 && l2 > 0 && l0 < l1 + l2 && l1 < l2 + l0 && l2 < l0 + l1))
      return tsl_fail("tsl_set_param: StVK membrane: rest lengths (%g, %g, %g) of face %d (cloth %d, face %d of the cloth) violate the triangle inequality", l0, l1, l2, f,
                      cid[f], f - c->h_cloth[cid[f]].face_start);
    const double a = (l0 * l0 + l2 * l2 - l1 * l1) / (2.0 * l0), b = sqrt(l2 * l2 - a * a);
    dm[4 * f] = 1.0 / l0; dm[4 * f + 1] = -a / (l0 * b); dm[4 * f + 2] = 0.0; dm[4 * f + 3] = 1.0 / b;
  }
  return c->cf_dminv.upload(dm);
}

// "cloth<i>.membrane" (0 springs + area term, 1 StVK), "cloth<i>.stvk_mu", "cloth<i>.stvk_lam"
static int stvk_set(tsl_ctx* c, const char* key, long idx, const std::string& f, double v) {
  const int n_cloth = (int)c->h_cloth.size();
  if (f == "membrane") {
    if (v != 0.0 && v != 1.0) return tsl_fail("tsl_set_param: %s must be 0 or 1 (got %g)", key, v);
    if (v == 1.0) TSL_TRY(stvk_prepare(c));
  }
  if (c->h_stvk.empty()) {
    c->h_stvk.assign(4 * (size_t)n_cloth, 0.0);
    TSL_TRY(c->d_stvk.alloc(c->h_stvk.size()));
  }
  c->h_stvk[4 * idx + (f == "membrane" ? 0 : (f == "stvk_mu" ? 1 : 2))] = v;
  c->n_stvk = 0;
  for (int i = 0; i < n_cloth; i++) c->n_stvk += c->h_stvk[4 * i] != 0.0;
  HIP_OK(hipMemcpy(c->d_stvk.p, c->h_stvk.data(), c->h_stvk.size() * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}

// "self_contact<body>" (geometry_self.projection_query(self_contact=[...])), "cloth<i>.Kb|Kl|Ka|k_angle|membrane|stvk_mu|stvk_lam",
// "elastic<i>.mu|lam|alpha" (0-d field writes after the context exists): one parser (param_keys.hpp), one table from field to member per family
static int set_indexed_param(tsl_ctx* c, const char* key, double v) {
  static const std::pair<const char*, double ClothDev::*> cloth_fields[] = {{"Kb", &ClothDev::Kb}, {"Kl", &ClothDev::Kl}, {"Ka", &ClothDev::Ka}, {"k_angle", &ClothDev::k_angle}};
  static const std::pair<const char*, double ElasticDev::*> elastic_fields[] = {{"mu", &ElasticDev::mu}, {"lam", &ElasticDev::lam}, {"alpha", &ElasticDev::alpha}};
  IndexedKey ik;
  if (parse_indexed_key(key, ik)) return tsl_fail("tsl_set_param: bad index in %s", key);
  const long idx = ik.index;
  const std::string& f = ik.field;
  if (ik.family == IndexedKey::SelfContact) {
    if (idx < 0 || idx >= c->n_body) return tsl_fail("tsl_set_param: bad body index in %s", key);
    if ((long)c->self_contact.size() < c->n_body) c->self_contact.assign(c->n_body, 0);
    c->self_contact[idx] = (v != 0.0);
  } else if (ik.family == IndexedKey::Cloth) {
    if (idx < 0 || idx >= (long)c->h_cloth.size()) return tsl_fail("tsl_set_param: bad cloth index in %s", key);
    if (f == "membrane" || f == "stvk_mu" || f == "stvk_lam") return stvk_set(c, key, idx, f, v);
    const auto* m = field_find(cloth_fields, f);
    if (!m) return tsl_fail("tsl_set_param: unknown key %s", key);
    c->h_cloth[idx].*(*m) = v;
    HIP_OK(hipMemcpy(c->d_cloth.p, c->h_cloth.data(), c->h_cloth.size() * sizeof(ClothDev), hipMemcpyHostToDevice));
  } else if (ik.family == IndexedKey::Elastic) {
    if (idx < 0 || idx >= (long)c->h_el.size()) return tsl_fail("tsl_set_param: bad elastic index in %s", key);
    const auto* m = field_find(elastic_fields, f);
    if (!m) return tsl_fail("tsl_set_param: unknown key %s", key);
    c->h_el[idx].*(*m) = v;
    HIP_OK(hipMemcpy(c->d_el.p, c->h_el.data(), c->h_el.size() * sizeof(ElasticDev), hipMemcpyHostToDevice));
    c->bd_valid = false;
  } else return tsl_fail("tsl_set_param: unknown key %s", key);
  return 0;
}

extern "C" int tsl_set_param(tsl_ctx* c, const char* key, double v) {
  Scope scope(c);
  (void)hipStreamSynchronize(c->stream);
  c->mg_omega_valid = false;
  c->ds.anorm_valid = false;   // any key may change the scale of the operator (materials, contact stiffness): |H|_inf is formed again when a refinement asks for it
  std::string k(key);
  if (k == "mu_cloth_elastic") c->mu_cloth_elastic = v;
  else if (k == "mu_cloth_cloth") c->mu_cloth_cloth = v;
  else if (k == "k_contact") c->k_contact = v;
  else if (k == "eps_contact") c->eps_contact = v;
  else if (k == "eps_v") c->eps_v = v;
  else if (k == "damping") c->damping = v;
  else if (k == "k_handle") {
    if (!(v >= 0.0) || !std::isfinite(v)) return tsl_fail("tsl_set_param: k_handle must be finite and >= 0 (got %g)", v);
    c->k_handle = v;
  }
  else if (k == "k_tie") {
    if (!(v >= 0.0) || !std::isfinite(v)) return tsl_fail("tsl_set_param: k_tie must be finite and >= 0 (got %g)", v);
    c->k_tie = v;
    TSL_TRY(tie_slots_refresh(c));   // (the tie slots exist while k_tie != 0)
  }
  else if (k == "k_collider" || k == "k_sphere" || k == "k_capsule" || k == "k_box" || k == "k_sdf") {
    if (!(v >= 0.0) || !std::isfinite(v)) return tsl_fail("tsl_set_param: %s must be finite and >= 0 (got %g)", key, v);
    (k == "k_collider" ? c->col.k : k == "k_sphere" ? c->sph.k : k == "k_capsule" ? c->cap.k : k == "k_box" ? c->box.k : c->sdf.k) = v;
  }
  else if (k == "wind_cn" || k == "wind_ct") {
    if (!(v >= 0.0) || !std::isfinite(v)) return tsl_fail("tsl_set_param: %s must be finite and >= 0 (got %g)", key, v);
    (k == "wind_cn" ? c->wind.cn : c->wind.ct) = v;
  }
  else if (k == "cg_tol") c->cg_tol = v;
  else if (k == "cg_maxit") c->cg_maxit = (int)v;
  else if (k == "newton_cap") c->newton_cap = (int)v;
  else if (k == "plastic") c->plastic = (int)v;
  else if (k == "spd_literal") {
    if (v != 0.0 && v != 1.0) return tsl_fail("tsl_set_param: spd_literal must be 0 or 1 (got %g)", v);
    c->spd_literal = (int)v;
  }
  else if (k == "contact") c->contact_enable = (v != 0.0);
  else if (k == "contact_ee") {
    if (v != 0.0 && v != 1.0) return tsl_fail("tsl_set_param: contact_ee must be 0 or 1 (got %g)", v);
    c->contact_ee = (int)v;
    if (c->contact_ee) TSL_TRY(ee_prepare(c));
  }
  else if (k == "grid_h") c->grid_h = v;
  else if (k == "grid_extent") c->grid_extent = v;
  else if (k == "adj_spd_pc") c->adj_spd_pc = (int)v;
  else if (k == "adj_clamp") c->adj_clamp = v;
  else if (k == "adj_clamp_angleref") c->adj_clamp_angleref = (int)v;
  else if (k == "verbose") c->verbose = (int)v;
  else if (k == "direct") { c->ds.enable = (int)v; c->ds.numeric_valid = false; c->ds.hard = false; }
  else if (k == "direct_berr") c->ds.berr_tol = v;
  else if (k == "direct_small_rounds") { c->ds.small_rounds = std::max(1, (int)v); c->ds.plan_valid = false; c->ds.numeric_valid = false; c->ds.cache.clear(); }
  else if (k == "tet_warm") c->tet_warm = (int)v;
  else if (k == "ds_dbg") c->ds.dbg = (int)v;
  else if (k == "ds_bench_batch") c->ds.bench_batch = (int)v;
  else if (k == "direct_flow") c->ds.flow = std::max(0, (int)v);
  else if (k == "direct_flow_token") { if (v == 0) ds_flow_token_release(c->ds); }   // 0: hand the device's dataflow token back (asked for again at the next eligible factorisation)
  else if (k == "direct_gemv_wide_below") c->ds.gemv_wide_below = std::max(0, (int)v);
  else if (k == "direct_g32_below") c->ds.g32_below = std::max(0, (int)v);
  else if (k == "direct_lookahead") c->ds.lookahead = (int)v;
  else if (k == "direct_piv_tol") { c->ds.piv_tol = v; c->ds.numeric_valid = false; }
  else if (k == "direct_leaf") { c->ds.leaf = std::max(4, (int)v); c->ds.static_ready = false; c->ds.plan_valid = false; c->ds.numeric_valid = false; }
  else if (k == "gmres_m") c->gmres_m = (int)v;
  else if (k == "body_inv") { c->bd_enable = (int)v; c->bd_valid = false; }
  else if (k == "mg") c->mg_enable = (int)v;
  else if (k == "mg_coarse_exact") { c->mg_coarse_exact = (int)v; c->mg_ops_valid = false; }   // (the hierarchy may end at another level)
  else if (k == "mg_dense_nodes") { c->mg_dense_auto = v < 0; if (v >= 0) c->mg_dense_nodes = (int)v; c->mg_ops_valid = false; }
  else return set_indexed_param(c, key, v);
  return 0;
}

extern "C" int tsl_set_frozen(tsl_ctx* c, const int32_t* fr) {
  Scope scope(c);
  (void)hipStreamSynchronize(c->stream);
  c->h_frozen.assign(fr, fr + 3 * (size_t)c->NV);
  c->mg_omega_valid = false;
  TSL_TRY(upload_frozen(c));
  if (c->pcg_graph) { (void)hipGraphExecDestroy(c->pcg_graph); c->pcg_graph = nullptr; }
  if (c->mr_graph) { (void)hipGraphExecDestroy(c->mr_graph); c->mr_graph = nullptr; }
  return body_dense_setup(c);
}
extern "C" int tsl_set_ext_force(tsl_ctx* c, const double* f) {
  Scope scope(c);
  (void)hipStreamSynchronize(c->stream);
  HIP_OK(hipMemcpy(c->fext.p, f, 3 * (size_t)c->NV * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}
extern "C" int tsl_set_gravity(tsl_ctx* c, const double* g) {
  Scope scope(c);
  (void)hipStreamSynchronize(c->stream);
  HIP_OK(hipMemcpy(c->grav.p, g, 3 * (size_t)c->NV * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}

// ------------------------------------------------------------------------------------------------
static CgScal* SC(tsl_ctx* c) { return (CgScal*)c->scal.p; }
static CgScal* HSC(tsl_ctx* c) { return (CgScal*)c->h_scal; }

static int energy_async(tsl_ctx* c, const double* pos, const double* prev, const double* vel, const double* ref) {
  hipStream_t s = c->stream;
  if (c->n_cface) hipLaunchKernelGGL(k_cloth_normals, dim3(nblk(c->n_cface, 256)), dim3(256), 0, s, c->n_cface, pos, c->cf_f2v.p, c->norm_dir.p);
  const int nmax = std::max(std::max(c->NV, c->n_cface), std::max(c->n_hinge, c->n_tet));
  // partials per workgroup, added in a fixed order (the line search decides on E < E0)
  const int nvf = contact_nvf(c);
  const int nb1 = nblk(nmax, 256), nb2 = nvf > 0 ? nblk(nvf, 64) : 0, nb3 = c->nc_ee > 0 ? nblk(c->nc_ee, 64) : 0;
  const int nb4 = handles_on(c) ? nblk(c->n_handle, 256) : 0;   // soft handles: their partials behind the contact ones
  const int nb5 = ties_on(c) ? nblk(c->n_tie, 64) : 0;          // ties: one partial per wave, behind the handle ones
  const size_t n_part = (size_t)nb1 + (size_t)nblk(c->max_n_constraints, 64) + 1 + (size_t)nblk(c->n_handle, 256) + (size_t)nblk(c->n_tie, 64) + (size_t)shapes_present(c) * shape_nblk(c) + (size_t)wind_nblk(c);
  if (c->e_part.n < n_part) { if (c->e_part.alloc(n_part)) return -1; }
  if (c->n_stvk > 0) hipLaunchKernelGGL(k_energy_stvk, dim3(nb1), dim3(256), 0, s, vert_args(c), cloth_args(c), tet_args(c), pos, prev, vel, ref, c->e_part.p, stvk_args(c));
  else hipLaunchKernelGGL(k_energy, dim3(nb1), dim3(256), 0, s, vert_args(c), cloth_args(c), tet_args(c), pos, prev, vel, ref, c->e_part.p);
  if (nb2 > 0) hipLaunchKernelGGL(k_contact_energy, dim3(nb2), dim3(64), 0, s, nvf, contact_args(c), pos, c->e_part.p + nb1);
  if (nb3 > 0) hipLaunchKernelGGL(k_ee_energy, dim3(nb3), dim3(64), 0, s, c->nc_ee, ee_args(contact_args(c), nvf), pos, c->e_part.p + nb1 + nb2);
  if (nb4 > 0) handle_dispatch(c, [&](auto NC) { hipLaunchKernelGGL(k_handle_energy<NC>, dim3(nb4), dim3(256), 0, s, handle_args(c), pos, c->e_part.p + nb1 + nb2 + nb3); });
  if (nb5 > 0) hipLaunchKernelGGL(k_tie_energy, dim3(nblk(c->n_tie, 256)), dim3(256), 0, s, tie_args(c), pos, c->e_part.p + nb1 + nb2 + nb3 + nb4);
  // colliders: one partial per workgroup of 256 vertices and kind (planes, balls, rods), behind the tie ones
  const int nb6 = shapes_energy_launch(c, s, pos, prev, c->e_part.p + nb1 + nb2 + nb3 + nb4 + nb5);
  // wind: one partial per workgroup of 256 listed faces, behind the colliders'
  const int nb7 = wind_energy_launch(c, s, pos, prev, c->e_part.p + nb1 + nb2 + nb3 + nb4 + nb5 + nb6);
  hipLaunchKernelGGL(k_energy_final, dim3(1), dim3(256), 0, s, nb1 + nb2 + nb3 + nb4 + nb5 + nb6 + nb7, (const double*)c->e_part.p, &SC(c)->energy);
  return 0;
}
static int energy_sync(tsl_ctx* c, const double* pos, const double* prev, const double* vel, const double* ref, double* E) {
  TSL_TRY(energy_async(c, pos, prev, vel, ref));
  HIP_OK(hipMemcpyAsync(&HSC(c)->energy, &SC(c)->energy, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  *E = HSC(c)->energy;
  return 0;
}

extern "C" int tsl_energy(tsl_ctx* c, const double* pos, const double* prev, const double* vel, const double* ref, double* E) {
  Scope scope(c);
  return energy_sync(c, pos, prev, vel, ref, E);
}

// The face kernels of an assembly: the <STVK> instantiations only while some cloth has membrane = 1, else the spring ones as they were
static void cloth_grad_face_launch(tsl_ctx* c, hipStream_t s, const ClothArgs& CA, const double* pos) {
  if (c->n_stvk > 0) hipLaunchKernelGGL(k_cloth_grad_face<true>, dim3(nblk(c->n_cface, 256)), dim3(256), 0, s, CA, pos, stvk_args(c));
  else hipLaunchKernelGGL(k_cloth_grad_face<false>, dim3(nblk(c->n_cface, 256)), dim3(256), 0, s, CA, pos, stvk_args(c));
}
// The gathers of the element staging slots and records, and the checks around them: each spelled once, for every assembly, read-out and reverse step
static int ensure_vg_stage(tsl_ctx* c) {   // the staging slots of the element gradients exist (allocated at the first use)
  const size_t n = 3 * (size_t)std::max(c->vg_ns, 1);
  if (c->vg_stage.n < n && c->vg_stage.alloc(n)) return tsl_fail("out of device memory (gradient staging)");
  return 0;
}
// out[v] += the three-vectors of v's staging slots in [lo, hi), ascending; stage: where slot 0 of the staging array is (or would be)
static void vertex_gather_launch(tsl_ctx* c, hipStream_t s, const double* stage, int lo, int hi, double* out) {
  hipLaunchKernelGGL(k_vertex_gather, dim3(nblk(c->NV, 256)), dim3(256), 0, s, c->NV, (const int*)c->vg_ptr.p, (const int*)c->vg_idx.p, stage, lo, hi, out);
}
// the element records summed into the matrix blocks [first_block, first_block + n_blocks) of the gather lists (cloth blocks first, body blocks behind them)
static void cloth_gather_launch(tsl_ctx* c, hipStream_t s, int first_block, int n_blocks) {
  hipLaunchKernelGGL(k_cloth_gather, dim3(nblk(n_blocks, CG_BPW)), dim3(256), 0, s, n_blocks, c->cg_base.p + first_block, c->cg_ptr.p + first_block, (const unsigned*)c->cg_ent.p,
                     c->n_hinge, c->n_cface, (const double*)c->cg_hrec.p, (const double*)c->cg_frec.p, (const double*)c->cg_trec.p, c->vals_full.p);
}
// The tail of both assembly schedules.  The block-Jacobi inverse belongs to the iterative hierarchy: a solve that goes to the factorisation never reads it
// (9 us + one dependent launch per Newton iteration of the direct path); solve_perm forms it when the hierarchy runs after all (block_jacobi_ensure)
static int block_jacobi_after_assembly(tsl_ctx* c) {
  if (c->pc_frozen) return 0;
  if (direct_takes_solve(c)) { c->dinv_valid = false; return 0; }
  return block_jacobi_refresh(c);
}
static void cloth_hess_face_launch(tsl_ctx* c, hipStream_t s, const ClothArgs& CA, const double* pos, const double* ref, int spd) {
  const dim3 g(nblk(c->n_cface, 128)), b(128);
  const StvkArgs S = stvk_args(c);
  const bool lit = c->spd_literal && spd == 1;
  if (c->n_stvk > 0) {
    if (spd == 2) hipLaunchKernelGGL((k_cloth_hess_face<true, false, true>), g, b, 0, s, CA, pos, ref, c->quirk.p, spd, c->cg_frec.p, S);
    else if (lit) hipLaunchKernelGGL((k_cloth_hess_face<false, true, true>), g, b, 0, s, CA, pos, ref, c->quirk.p, spd, c->cg_frec.p, S);
    else hipLaunchKernelGGL((k_cloth_hess_face<false, false, true>), g, b, 0, s, CA, pos, ref, c->quirk.p, spd, c->cg_frec.p, S);
  } else {
    if (spd == 2) hipLaunchKernelGGL((k_cloth_hess_face<true>), g, b, 0, s, CA, pos, ref, c->quirk.p, spd, c->cg_frec.p, S);
    else if (lit) hipLaunchKernelGGL((k_cloth_hess_face<false, true>), g, b, 0, s, CA, pos, ref, c->quirk.p, spd, c->cg_frec.p, S);
    else hipLaunchKernelGGL((k_cloth_hess_face<false>), g, b, 0, s, CA, pos, ref, c->quirk.p, spd, c->cg_frec.p, S);
  }
}

// GPU work of one assembly (no host state, no allocation: assemble() below prepares both, so that the launches can be captured into a graph)
static int assemble_enqueue_early(tsl_ctx* c, const double* pos, const double* prev, const double* vel, const double* ref, int spd, double* grad, int tet_warm_flag);
static int assemble_enqueue(tsl_ctx* c, const double* pos, const double* prev, const double* vel, const double* ref, int spd, double* grad, int tet_warm_flag) {
  hipStream_t s = c->stream;
  const int NV = c->NV;
  if (c->nc > 0 || c->n_tet > 0) return assemble_enqueue_early(c, pos, prev, vel, ref, spd, grad, tet_warm_flag);
  // a bare cloth: one stream
  HIP_OK(hipMemsetAsync(c->vals_full.p, 0, c->vals_full.n * sizeof(double), s));
  if (c->n_cface) hipLaunchKernelGGL(k_cloth_normals, dim3(nblk(c->n_cface, 256)), dim3(256), 0, s, c->n_cface, pos, c->cf_f2v.p, c->norm_dir.p);
  ClothArgs CA = cloth_args(c);
  const VertArgs VA = vert_args(c);
  CA.gstage = c->vg_stage.p;   // element gradients into staging slots, element blocks into records: summed by k_vertex_gather / k_cloth_gather in a fixed order
  if (grad) {
    HIP_OK(hipMemsetAsync(grad, 0, 3 * (size_t)NV * sizeof(double), s));
    hipLaunchKernelGGL(k_vert_grad, dim3(nblk(NV, 256)), dim3(256), 0, s, VA, pos, prev, vel, grad);
  }
  hipLaunchKernelGGL(k_vert_hess, dim3(nblk(NV, 256)), dim3(256), 0, s, VA, c->diag_blk.p, c->vals_full.p);      // (the mass diagonal: the first contribution to its blocks)
  handle_assemble_launch(c, s, pos, grad);
  shapes_assemble_launch(c, s, spd, pos, prev, grad);
  wind_assemble_launch(c, s, pos, prev, grad);
  if (grad) {
    if (c->n_cface) cloth_grad_face_launch(c, s, CA, pos);
    if (c->n_hinge) hipLaunchKernelGGL(k_cloth_grad_hinge, dim3(nblk(c->n_hinge, 256)), dim3(256), 0, s, CA, pos, ref);
  }
  if (c->n_cface) {
    const int nq = (int)c->h_cloth.size() * 9;
    hipLaunchKernelGGL(k_cloth_quirk, dim3(nblk(nq, 64)), dim3(64), 0, s, CA, (int)c->h_cloth.size(), pos, ref, c->quirk.p);
    cloth_hess_face_launch(c, s, CA, pos, ref, spd);
  }
  if (c->n_hinge) hipLaunchKernelGGL(k_cloth_hess_hinge, dim3(nblk(c->n_hinge, 256)), dim3(256), 0, s, CA, pos, c->cg_hrec.p);
  if (c->n_cgblk_cloth > 0) cloth_gather_launch(c, s, 0, c->n_cgblk_cloth);
  if (grad) {
    vertex_gather_launch(c, s, c->vg_stage.p, 0, c->vg_ns, grad);
    hipLaunchKernelGGL(k_mask_vec, dim3(gsz(3 * (size_t)NV)), dim3(256), 0, s, 3 * (size_t)NV, c->frozen.p, grad);
  }
  hipLaunchKernelGGL(k_mask_matrix, dim3(c->n_slices), dim3(256), 0, s, c->n_slices, c->slice_off.p, c->slice_len.p, c->colidx.p, c->fzmask.p, c->mdt2.p,
                     c->vals_full.p, c->vals.p, NV);
  TSL_TRY(block_jacobi_after_assembly(c));
  HIP_OK(hipGetLastError());
  return 0;
}

// The deterministic assembly with bodies or contacts (the default of every scene but a bare cloth): the element, hinge and contact kernels only
// STORE (staging slots of the gradient, element records of the matrix), so the three streams depend on each other in few places, and the
// HOST paces an assembly -- it starts right after the line search's energy was read back, every queue empty, and issues ~35 launches of
// 5-120 us at 6-8 us each.  Issue order = priority order: the long kernel of every chain first, then the short ones.
//   element stream:  tet gradients, tet blocks (110 us) | after the mass diagonal: body blocks gathered
//   engine stream:   clear, normals, vertex terms, quirk, face blocks (90 us), hinge blocks (records, 30 us), cloth blocks gathered | after the body blocks: mask,
//                    block-Jacobi
//   contact stream:  contact blocks (120 us), mask, diagonal | hinge gradients, face gradients | after the tet gradients: vertex gather, contact rows, mask
// (round 4 traces, cfg4: the engine stream's first cloth kernel started 200 us after the assembly's first launch and its chain -- face blocks,
// hinge blocks, gather, then the gradient tail and the matrix tail one after the other -- ended 580 us after the energy read-back; then ~440.  Round 5: the
// hinge blocks and the face gradients sat on the element stream behind the bodies' element blocks and held back both gathers: moved, -1.8 % of a step.
// A fourth stream for the gradient chain and the engine stream's head issued first were measured slower: DESIGN.md 9b.)
static int assemble_enqueue_early(tsl_ctx* c, const double* pos, const double* prev, const double* vel, const double* ref, int spd, double* grad, int tet_warm_flag) {
  hipStream_t s = c->stream, st = c->side;
  const bool fork_t = c->n_tet > 0 && c->nc > 0;
  hipStream_t stt = fork_t ? c->side2 : st;
  const int NV = c->NV;
  ClothArgs CA = cloth_args(c);
  const VertArgs VA = vert_args(c);
  TetArgs TA = tet_args(c);
  CA.gstage = c->vg_stage.p; TA.gstage = c->vg_stage.p + 3 * (size_t)c->vg_tet0;
  HIP_OK(hipEventRecord(c->ev_fork0, s));   // (whatever the caller queued on the engine stream before -- positions -- comes first)
  HIP_OK(hipStreamWaitEvent(st, c->ev_fork0, 0));
  if (fork_t) HIP_OK(hipStreamWaitEvent(stt, c->ev_fork0, 0));
  TSL_TRY(contact_assemble(c, pos, spd, grad, st));   // (the longest chain: blocks 120-160 us, mask, diagonal, hinge gradients, gradient tail)
  const bool gather = c->n_cgblk > 0;
  const bool hh_side = fork_t && gather;
  // element stream: the hinge blocks first (records: they read positions only), so that the cloth gather on the engine stream can start when the face blocks end
  if (hh_side && c->n_hinge) {
    hipLaunchKernelGGL(k_cloth_hess_hinge, dim3(nblk(c->n_hinge, 256)), dim3(256), 0, stt, CA, pos, c->cg_hrec.p);
    HIP_OK(hipEventRecord(c->ev_hh, stt));
  }
  if (c->n_tet) {
    if (grad) { hipLaunchKernelGGL(k_tet_grad, dim3(nblk(c->n_tet, 256)), dim3(256), 0, stt, TA, pos); HIP_OK(hipEventRecord(c->ev_g2, stt)); }   // tet gradients staged
    // eigen-clamp of the element blocks warm-started from the previous assembly's eigenvectors ("tet_warm", on by default);
    // every 16th clamped assembly starts from the identity again (orthogonality of the accumulated rotations)
    // ("spd_literal": the reference's projector on the blocks as formed, no basis)
    const bool lit = c->spd_literal && spd == 1;
    double* vws = (c->tet_warm && spd != 0 && !lit) ? c->tet_V.p : (double*)nullptr;   // (allocated and counted by assemble())
    if (lit) hipLaunchKernelGGL(k_tet_hess_coop<true>, dim3(nblk(c->n_tet, 16)), dim3(256), 0, stt, TA, pos, spd, vws, 0, c->cg_trec.p);
    else hipLaunchKernelGGL(k_tet_hess_coop<false>, dim3(nblk(c->n_tet, 16)), dim3(256), 0, stt, TA, pos, spd, vws, vws ? tet_warm_flag : 0, c->cg_trec.p);
  }
  HIP_OK(hipMemsetAsync(c->vals_full.p, 0, c->vals_full.n * sizeof(double), s));
  if (c->n_cface) hipLaunchKernelGGL(k_cloth_normals, dim3(nblk(c->n_cface, 256)), dim3(256), 0, s, c->n_cface, pos, c->cf_f2v.p, c->norm_dir.p);
  if (grad) {
    HIP_OK(hipMemsetAsync(grad, 0, 3 * (size_t)NV * sizeof(double), s));
    hipLaunchKernelGGL(k_vert_grad, dim3(nblk(NV, 256)), dim3(256), 0, s, VA, pos, prev, vel, grad);
  }
  hipLaunchKernelGGL(k_vert_hess, dim3(nblk(NV, 256)), dim3(256), 0, s, VA, c->diag_blk.p, c->vals_full.p);   // (the mass diagonal: the first contribution to its blocks)
  handle_assemble_launch(c, s, pos, grad);   // (on the stream of the vertex terms, in front of ev_fork: the gathers and masks of the other streams wait for it as they do for those)
  shapes_assemble_launch(c, s, spd, pos, prev, grad);
  wind_assemble_launch(c, s, pos, prev, grad);
  HIP_OK(hipEventRecord(c->ev_fork, s));   // normals, vertex gradient and mass diagonal are in place
  if (c->n_cface) {
    const int nq = (int)c->h_cloth.size() * 9;
    hipLaunchKernelGGL(k_cloth_quirk, dim3(nblk(nq, 64)), dim3(64), 0, s, CA, (int)c->h_cloth.size(), pos, ref, c->quirk.p);
    cloth_hess_face_launch(c, s, CA, pos, ref, spd);
  }
  // element stream, second part (behind the normals and the mass diagonal).  Round 6: the element blocks of the bodies take 55 us since they are formed by 16 lanes
  // per element (k_tet_hess_coop; 170 before), so the hinge blocks (records, 45-60 us) run HERE, next to the face blocks on the engine stream, and the face
  // gradients behind the body blocks: the engine stream's chain is face blocks -> cloth gather -> mask, the contact stream's contact blocks -> hinge gradients ->
  // gradient tail.  (Round 5 had moved them the other way, when this stream was busy with the bodies for 170 us.)
  HIP_OK(hipStreamWaitEvent(stt, c->ev_fork, 0));
  if (c->n_hinge && !hh_side) hipLaunchKernelGGL(k_cloth_hess_hinge, dim3(nblk(c->n_hinge, 256)), dim3(256), 0, s, CA, pos, c->cg_hrec.p);
  const int nt_blk = c->n_cgblk - c->n_cgblk_cloth;
  if (c->n_tet && nt_blk > 0)   // the element records of the bodies -> their matrix blocks (the blocks of the bodies and of the cloth are disjoint)
    cloth_gather_launch(c, stt, c->n_cgblk_cloth, nt_blk);
  HIP_OK(hipEventRecord(c->ev_join2, stt));   // body blocks
  // contact stream, second part: hinge gradients (staging slots); the face gradients behind the body blocks on the element stream
  if (grad) {
    if (fork_t) HIP_OK(hipStreamWaitEvent(st, c->ev_fork, 0));
    if (c->n_hinge) hipLaunchKernelGGL(k_cloth_grad_hinge, dim3(nblk(c->n_hinge, 256)), dim3(256), 0, st, CA, pos, ref);
    if (c->n_cface) {
      cloth_grad_face_launch(c, hh_side ? stt : st, CA, pos);
      if (hh_side) HIP_OK(hipEventRecord(c->ev_gf, stt));
    }
  }
  // engine stream: cloth blocks (behind the hinge records), then the matrix tail
  if (hh_side && c->n_hinge) HIP_OK(hipStreamWaitEvent(s, c->ev_hh, 0));
  if (gather && c->n_cgblk_cloth > 0) cloth_gather_launch(c, s, 0, c->n_cgblk_cloth);
  HIP_OK(hipStreamWaitEvent(s, c->ev_join2, 0));
  hipLaunchKernelGGL(k_mask_matrix, dim3(c->n_slices), dim3(256), 0, s, c->n_slices, c->slice_off.p, c->slice_len.p, c->colidx.p, c->fzmask.p, c->mdt2.p,
                     c->vals_full.p, c->vals.p, NV);
  // contact stream: the gradient tail
  if (grad) {
    if (fork_t && c->n_tet) HIP_OK(hipStreamWaitEvent(st, c->ev_g2, 0));
    if (hh_side && c->n_cface) HIP_OK(hipStreamWaitEvent(st, c->ev_gf, 0));
    vertex_gather_launch(c, st, c->vg_stage.p, 0, c->vg_ns, grad);
    if (c->nc > 0) hipLaunchKernelGGL(k_contact_row_gather, dim3(nblk((long)NV * 64, 256)), dim3(256), 0, st, NV, (const int*)c->rowpos.p, (const int*)c->cr_ptr.p, (const int*)c->cr_ent.p,
                                      (const double*)c->c_G.p, grad);
    hipLaunchKernelGGL(k_mask_vec, dim3(gsz(3 * (size_t)NV)), dim3(256), 0, st, 3 * (size_t)NV, c->frozen.p, grad);
  }
  HIP_OK(hipEventRecord(c->ev_join, st));
  HIP_OK(hipStreamWaitEvent(s, c->ev_join, 0));   // (contact diagonal for the block-Jacobi inverse, the gradient for whatever follows)
  TSL_TRY(block_jacobi_after_assembly(c));
  HIP_OK(hipGetLastError());
  return 0;
}

// One assembly: host state and lazy allocations, then the ~45 launches on three streams.  Measured and dropped (round 4): the launches as ONE
// hipGraph launch keyed by the arguments (the 50 Newton iterations of a step call with the same ones) -- right after the host has read the
// line search's energy the GPU has nothing queued and the assembly's kernels are shorter than the host needs to issue them (a kernel
// trace shows the engine stream idle for 120 us in front of the first cloth kernel), but the replay of the three-stream graph is slower
// than the launches: 269.2 against 263.4 ms per step on the driver's command.
static int assemble(tsl_ctx* c, const double* pos, const double* prev, const double* vel, const double* ref, int spd, double* grad) {
  hipStream_t s = c->stream;
  // ---- allocations the launches rely on (staging slots of the gradient, element records of the matrix)
  TSL_TRY(ensure_vg_stage(c));
  if (c->n_tet > 0 && c->cg_trec.n < 144 * (size_t)c->n_tet) { if (c->cg_trec.alloc(144 * (size_t)c->n_tet)) return tsl_fail("out of device memory (element records)"); }
  if (grad && c->nc > 0 && c->c_G.n < 12 * contact_cap(c)) { if (c->c_G.alloc(12 * contact_cap(c))) return -1; }
  if (c->n_cgblk > 0 && c->n_cface > 0 && c->cg_frec.n == 0) {
    if (c->cg_hrec.alloc((size_t)std::max(c->n_hinge, 1) * 16) | c->cg_frec.alloc((size_t)c->n_cface * 81)) return tsl_fail("out of device memory (cloth element records)");
  }
  int warm = 0;
  if (c->n_tet > 0 && c->tet_warm && spd != 0 && !(c->spd_literal && spd == 1)) {   // (the literal projector keeps no basis)
    if (c->tet_V.n < (size_t)81 * c->n_tet) {
      if (c->tet_V.alloc((size_t)81 * c->n_tet)) return tsl_fail("out of device memory (tet eigenvectors)");
      HIP_OK(hipMemsetAsync(c->tet_V.p, 0, c->tet_V.n * sizeof(double), s));   // "no basis yet" for every element (spd_clamp_warm checks the norm)
      c->tet_V_count = 0;
    }
    warm = (c->tet_V_count++ % 16) != 0;   // every 16th clamped assembly starts from the identity again
  }
  // ---- host state
  c->st_pos = pos; c->st_prev = prev; c->st_vel = vel; c->st_ref = ref;  // for forward_spd_pc (valid while tsl_step runs)
  c->ds.numeric_valid = false;   // (|H|_inf, the yardstick of the backward errors, ages with the factorisations: direct_factor / group_solve)
  if (spd != c->ds.anorm_spd) { c->ds.anorm_valid = false; c->ds.anorm_spd = spd; }   // the un-projected adjoint operator does not borrow the forward operator's norm (and back)
  if (!c->pc_frozen) { c->mg_ops_valid = false; c->pc_separate = false; }
  return assemble_enqueue(c, pos, prev, vel, ref, spd, grad, warm);
}

extern "C" int tsl_assemble(tsl_ctx* c, const double* pos, const double* prev, const double* vel, const double* ref, int spd, double* grad) {
  Scope scope(c);
  c->bd_valid = false;
  c->mg_omega_valid = false;
  // an assembly from outside a step may hold any operator (a new scene state, a new scale): the backward errors of its solves are measured
  // against its own |H|_inf, not one kept from an earlier assembly (the 64-factorisation cache is for the Newton iterations inside tsl_step)
  c->ds.anorm_valid = false;
  return assemble(c, pos, prev, vel, ref, spd, grad);
}

// ------------------------------------------------------------------------------------------------
// y = H x in permuted space (matrix + matrix-free contact blocks); optional fused dot into pAp[slot]
// contact rows of the current constraint set with the given 12x12 blocks (ptr = null: no contacts)
static ContactRows contact_rows(tsl_ctx* c, const double* blocks) {
  ContactRows R;
  R.ptr = c->nc > 0 ? c->cr_ptr.p : (const int*)nullptr;
  R.ent = c->cr_ent.p; R.rows = c->cr_rows.p; R.H = blocks; R.nv = c->NV;
  return R;
}

static void launch_spmv(tsl_ctx* c, const double* vals, const double* x, double* y, int slot, int check_flag, bool full_contact = false) {
  hipStream_t s = c->stream;
  if (slot < 0 && !check_flag) {  // plain product (residuals, MINRES / GMRES / BiCGStab): multi-wave kernel with the contact rows folded in
    hipLaunchKernelGGL((k_spmv_mw<4, 1, TSL_NT>), dim3(c->n_slices), dim3(256), 0, s, c->NV, c->n_slices, c->slice_off.p, c->slice_len.p, c->colidx.p, vals, x, y,
                       (double*)nullptr, (const int*)nullptr, contact_rows(c, full_contact ? c->c_Hfull.p : c->c_H.p));
    return;
  }
  const bool sample = c->prof_enable && slot >= 0 && (c->prof_launches % 16 == 0) && c->ev_used < c->ev_pool.size();
  if (sample) (void)hipEventRecord(c->ev_pool[c->ev_used].first, s);
  unsigned long long* dprof = nullptr;
  if (c->prof_enable && slot >= 0 && (c->prof_launches % 64 == 40) && c->prof_dev_used < c->prof_dev_cap) dprof = c->prof_dev.p + 2 * c->prof_waves * (c->prof_dev_used++);
  hipLaunchKernelGGL(k_spmv, dim3(nblk((long)c->n_slices * 64, 256)), dim3(256), 0, s, c->NV, c->n_slices, c->slice_off.p, c->slice_len.p, c->colidx.p, vals, x, y,
                     SC(c), slot, check_flag, dprof);
  if (sample) { (void)hipEventRecord(c->ev_pool[c->ev_used].second, s); c->ev_used++; }
  if (slot >= 0) c->prof_launches++;
  if (c->nc > 0)
    hipLaunchKernelGGL(k_contact_matvec, dim3(nblk(c->nc, 64)), dim3(CONTACT_MV_THREADS), 0, s, c->nc, c->c_idx.p, c->rowpos.p, full_contact ? c->c_Hfull.p : c->c_H.p, x, y, SC(c), slot,
                       check_flag);
}

// The product kernels that tsl_bench_spmv times (variants 0..7: k_spmv with the fused dot into pAp[0], six instantiations of k_spmv_mw on the static
// matrix with their per-workgroup dot partials), launched once: one place for the timing and for tsl_op_apply (op_test_api.hpp), which checks what they
// return.  Returns the number of partials the launch writes (its grid; 0: the dot goes to pAp[0]), -1 for another variant.
static int spmv_variant_launch(tsl_ctx* c, int variant, const double* x, double* y, double* part) {
  hipStream_t s = c->stream;
  const int ns = c->n_slices;
  switch (variant) {
    case 0: hipLaunchKernelGGL(k_spmv, dim3(nblk((long)ns * 64, 256)), dim3(256), 0, s, c->NV, ns, c->slice_off.p, c->slice_len.p, c->colidx.p, c->vals.p, x, y, SC(c), 0, 0, (unsigned long long*)nullptr); break;
    case 1: hipLaunchKernelGGL((k_spmv_mw<1, 4, false>), dim3(nblk(ns, 4)), dim3(256), 0, s, c->NV, ns, c->slice_off.p, c->slice_len.p, c->colidx.p, c->vals.p, x, y, part, (const int*)nullptr, ContactRows{}); break;
    case 2: hipLaunchKernelGGL((k_spmv_mw<4, 1, false>), dim3(ns), dim3(256), 0, s, c->NV, ns, c->slice_off.p, c->slice_len.p, c->colidx.p, c->vals.p, x, y, part, (const int*)nullptr, ContactRows{}); break;
    case 3: hipLaunchKernelGGL((k_spmv_mw<4, 1, true>), dim3(ns), dim3(256), 0, s, c->NV, ns, c->slice_off.p, c->slice_len.p, c->colidx.p, c->vals.p, x, y, part, (const int*)nullptr, ContactRows{}); break;
    case 4: hipLaunchKernelGGL((k_spmv_mw<2, 2, false>), dim3(nblk(ns, 2)), dim3(256), 0, s, c->NV, ns, c->slice_off.p, c->slice_len.p, c->colidx.p, c->vals.p, x, y, part, (const int*)nullptr, ContactRows{}); break;
    case 5: hipLaunchKernelGGL((k_spmv_mw<8, 1, false>), dim3(ns), dim3(512), 0, s, c->NV, ns, c->slice_off.p, c->slice_len.p, c->colidx.p, c->vals.p, x, y, part, (const int*)nullptr, ContactRows{}); break;
    case 6: hipLaunchKernelGGL((k_spmv_mw<4, 2, false>), dim3(nblk(ns, 2)), dim3(512), 0, s, c->NV, ns, c->slice_off.p, c->slice_len.p, c->colidx.p, c->vals.p, x, y, part, (const int*)nullptr, ContactRows{}); break;
    case 7: hipLaunchKernelGGL((k_spmv_mw<2, 2, true>), dim3(nblk(ns, 2)), dim3(256), 0, s, c->NV, ns, c->slice_off.p, c->slice_len.p, c->colidx.p, c->vals.p, x, y, part, (const int*)nullptr, ContactRows{}); break;
    default: return -1;
  }
  return variant == 0 ? 0 : variant == 1 ? nblk(ns, 4) : (variant == 4 || variant == 6 || variant == 7) ? nblk(ns, 2) : ns;
}

static void prof_collect(tsl_ctx* c) {
  for (size_t i = 0; i < c->ev_used; i++) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->ev_pool[i].first, c->ev_pool[i].second) == hipSuccess) { c->prof_ms += ms; c->prof_samples++; }
  }
  c->ev_used = 0;
}

static int read_scal(tsl_ctx* c) {
  HIP_OK(hipMemcpyAsync(c->h_scal, c->scal.p, sizeof(CgScal), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  if (c->prof_enable) prof_collect(c);
  return 0;
}

// does the next linear solve of this context go straight to the factorisation (solve_direct's rule, the probe of the automatic mode included)?
static bool direct_takes_solve(tsl_ctx* c) {
  const DirectSolver& d = c->ds;
  return direct_enabled(c) && !c->ds_suspended && !(d.enable < 0 && !d.hard && c->n_tet == 0 && c->nc == 0);
}
static int block_jacobi_refresh(tsl_ctx* c) {
  if (c->nc > 0 && !c->cdiag_valid) contact_diag_refresh(c, c->stream);   // (skipped by an assembly that expected the factorisation to take the solve)
  hipLaunchKernelGGL(k_block_jacobi, dim3(nblk(c->NV, 256)), dim3(256), 0, c->stream, c->NV, c->diag_perm.p, c->vals.p, c->nc > 0 ? c->c_diag.p : (const double*)nullptr, c->Dinv.p);
  if (body_active(c) && c->bd_valid) body_zero_dinv(c);  // those rows are served by the (lagged) dense inverse
  c->dinv_valid = true;
  return 0;
}
static int block_jacobi_ensure(tsl_ctx* c) { return c->dinv_valid ? 0 : block_jacobi_refresh(c); }

// ------------------------------------------------------------------------------------------------ dense body blocks (k_body.hpp)
// which elastic bodies get an exact block: at most 512 vertices, at least one free dof
static int body_dense_setup(tsl_ctx* c) {
  BodyDenseArgs& A = c->bd_args;
  A = BodyDenseArgs{};
  c->bd_valid = false; c->bd_rows_n = 0; c->bd_n3max = 0; c->bd_wg = 0; c->bd_scr_n = 0; c->bd_w_total = 0;
  std::vector<int> rows, body_of(c->NV, -1), local_of(c->NV, 0);
  for (const ElasticDev& e : c->h_el) {
    if (A.nb >= TSL_MAX_DENSE_BODIES || e.n_verts > 512 || e.n_verts < 2) continue;
    bool any_free = false;
    for (int v = e.v_offset; v < e.v_offset + e.n_verts && !any_free; v++)
      any_free = !(c->h_frozen[3 * v] && c->h_frozen[3 * v + 1] && c->h_frozen[3 * v + 2]);
    if (!any_free) continue;
    const int b = A.nb++;
    A.n3[b] = 3 * e.n_verts;
    A.rows_off[b] = (int)rows.size();
    A.w_off[b] = (long)c->bd_w_total;
    A.scr_off[b] = c->bd_scr_n;
    A.wg_off[b] = c->bd_wg;
    for (int k = 0; k < e.n_verts; k++) {
      const int v = e.v_offset + k;
      rows.push_back(c->h_rowpos[v]); body_of[v] = b; local_of[v] = k;
    }
    c->bd_w_total += (size_t)A.n3[b] * ((A.n3[b] + 3) & ~3);  // multiple of 4: every body block starts 16-byte aligned
    c->bd_scr_n += A.n3[b];
    c->bd_wg += (A.n3[b] + BODY_APPLY_ROWS - 1) / BODY_APPLY_ROWS;
    c->bd_n3max = std::max(c->bd_n3max, A.n3[b]);
  }
  A.wg_off[A.nb] = c->bd_wg;
  c->bd_rows_n = (int)rows.size();
  if (!A.nb) return 0;
  TSL_TRY(c->bd_rows.upload(rows)); TSL_TRY(c->bd_body_of.upload(body_of)); TSL_TRY(c->bd_local_of.upload(local_of));
  if (c->bd_bad.alloc(TSL_MAX_DENSE_BODIES) | c->bd_W.alloc(c->bd_w_total) | c->bd_Binv.alloc(c->bd_w_total) | c->bd_scr.alloc(4 * (size_t)c->bd_scr_n) | c->bd_rb.alloc(2 * (size_t)c->bd_scr_n)) return -1;
  A.rows = c->bd_rows.p; A.body_of = c->bd_body_of.p; A.local_of = c->bd_local_of.p;
  HIP_OK(hipMemsetAsync(c->bd_Binv.p, 0, c->bd_w_total * sizeof(float), c->stream));  // the row padding must stay finite (it multiplies zeros)
  return 0;
}

// auto (-1): only together with the cloth multigrid -- on the reference-size scenes the coarse 15x7 cloth, not the bodies,
// limits PCG and the dense apply (27 MB per sweep) costs more than it saves
static bool body_active(tsl_ctx* c) {
  if (c->bd_args.nb <= 0 || c->bd_enable == 0) return false;
  return c->bd_enable > 0 || (!c->mg.empty() && c->mg_enable != 0);
}

static void body_zero_dinv(tsl_ctx* c) {
  hipLaunchKernelGGL(k_body_zero_dinv, dim3(nblk(c->bd_rows_n, 256)), dim3(256), 0, c->stream, c->bd_args, c->bd_rows_n, c->Dinv.p);
}

// (re)build the dense inverses from the current masked matrix + contact blocks; Dinv must hold the point-Jacobi blocks
static int body_build_inverse(tsl_ctx* c) {
  hipStream_t s = c->stream;
  const BodyDenseArgs& A = c->bd_args;
  HIP_OK(hipMemsetAsync(c->bd_W.p, 0, c->bd_w_total * sizeof(double), s));
  HIP_OK(hipMemsetAsync(c->bd_bad.p, 0, TSL_MAX_DENSE_BODIES * sizeof(int), s));
  for (int b = 0; b < A.nb; b++)
    hipLaunchKernelGGL(k_body_gather, dim3(A.n3[b] / 3), dim3(64), 0, s, A, b, c->slice_off.p, c->slice_len.p, c->colidx.p, c->perm.p, c->vals.p, c->bd_W.p);
  if (c->nc > 0) hipLaunchKernelGGL(k_body_contact, dim3(nblk(c->nc, 64)), dim3(64), 0, s, A, c->nc, c->c_idx.p, c->c_H.p, c->bd_W.p);
  double* col[2] = {c->bd_scr.p, c->bd_scr.p + 2 * (size_t)c->bd_scr_n};
  double* row[2] = {c->bd_scr.p + c->bd_scr_n, c->bd_scr.p + 3 * (size_t)c->bd_scr_n};
  hipLaunchKernelGGL(k_body_gj_init, dim3(nblk(c->bd_n3max, 256), A.nb), dim3(256), 0, s, A, c->bd_W.p, col[0], row[0]);
  const dim3 grid(nblk((long)c->bd_n3max * c->bd_n3max, 256), A.nb);
  for (int k = 0; k < c->bd_n3max; k++)
    hipLaunchKernelGGL(k_body_gj, grid, dim3(256), 0, s, A, k, c->bd_W.p, col[k & 1], row[k & 1], col[(k & 1) ^ 1], row[(k & 1) ^ 1], c->bd_bad.p);
  hipLaunchKernelGGL(k_body_finalize, grid, dim3(256), 0, s, A, c->bd_W.p, c->bd_bad.p, c->Dinv.p, c->bd_Binv.p);
  body_zero_dinv(c);
  c->bd_valid = true;
  HIP_OK(hipGetLastError());
  return 0;
}

static void body_apply(tsl_ctx* c, int mode, const double* r, const double* t, double* z, const double* rdot, double* part) {
  hipLaunchKernelGGL(k_body_apply, dim3(c->bd_wg), dim3(256), 0, c->stream, c->bd_args, c->bd_Binv.p, mode, r, t, z, rdot, part);
}

// ------------------------------------------------------------------------------------------------ multigrid (k_mg.hpp)
static int mg_build(tsl_ctx* c, const tsl_scene_desc* d) {
  for (int ci = 0; ci < d->n_cloth; ci++) {
    const tsl_cloth_desc& cd = d->cloths[ci];
    int N = cd.N, M = cd.M;
    if (N < 8 || M < 8 || (N & 1) || (M & 1)) continue;
    MgCloth* mc = new MgCloth();
    mc->v_offset = cd.v_offset; mc->N0 = N; mc->M0 = M;
    while (!(N & 1) && !(M & 1) && std::min(N, M) >= 4) {
      N >>= 1; M >>= 1;
      MgLevel* L = new MgLevel();
      L->N = N; L->M = M; L->n = (N + 1) * (M + 1);
      int rc = L->A.alloc((size_t)225 * L->n) | L->Dinv.alloc((size_t)9 * L->n) | L->x.alloc((size_t)3 * L->n) | L->x2.alloc((size_t)3 * L->n) | L->r.alloc((size_t)3 * L->n) | L->t.alloc((size_t)3 * L->n) | L->omega.alloc(2);
      mc->lv.push_back(L);
      if (rc) { delete mc; return -1; }
    }
    c->mg.push_back(mc);
  }
  if (!c->mg.empty()) {
    if (c->mg_omega0.alloc(2) | c->mg_pi_part.alloc((size_t)c->NV / 256 + 8) | c->mg_pi_norm.alloc(64)) return -1;
  }
  return 0;
}

static size_t mg_levels(tsl_ctx* c, MgCloth* mc) {
  size_t nl = mc->lv.size();
  if (c->mg_coarse_exact)  // the hierarchy ends at the first level small enough for a dense inverse
    for (size_t l = 0; l < nl; l++)
      if (mc->lv[l]->n <= std::max(c->mg_dense_nodes, 1)) { nl = l + 1; break; }
  return nl;
}
static bool mg_level_dense(tsl_ctx* c, MgLevel* L) { return c->mg_coarse_exact && (L->n <= 64 || L->n <= c->mg_dense_nodes); }
static bool mg_active(tsl_ctx* c) { return !c->mg.empty() && c->mg_enable != 0 && !c->mg_suspended; }

// plain y = H x on level 0 (matrix + matrix-free contact), no scalar side effects.  The smoother products read the single-precision copy of the
// preconditioner's matrix (half the bytes): mg_setup_operators writes it before anything else, and every caller runs behind a set-up
// (mg_setup_operators itself, and mg_vcycle, which is only reached with mg_ops_valid).
static void mg_spmv0(tsl_ctx* c, const double* x, double* y) {
  const double* cH = c->pc_separate ? c->c_H_pc.p : c->c_H.p;
  hipLaunchKernelGGL((k_spmv_mw<4, 1, TSL_NT, float>), dim3(c->n_slices), dim3(256), 0, c->stream, c->NV, c->n_slices, c->slice_off.p, c->slice_len.p, c->colidx.p, c->vals32.p, x, y,
                     (double*)nullptr, (const int*)nullptr, contact_rows(c, cH));
}

// Galerkin coarse operators of the current (masked) matrix; called once per assembly when the preconditioner is active
static int mg_setup_operators(tsl_ctx* c) {
  hipStream_t s = c->stream;
  // the matrix in c->vals at this point is the one the preconditioner is built from (also in the separate-pc set-ups)
  if (c->vals32.n == 0 && c->vals32.alloc(c->vals.n)) return tsl_fail("out of device memory (vals32)");
  hipLaunchKernelGGL(k_vals_to_f32, dim3(gsz(c->vals.n)), dim3(256), 0, s, c->vals.n, c->vals.p, c->vals32.p);
  for (MgCloth* mc : c->mg) {
    MgGrid gf{mc->N0, mc->M0};
    MgLevel* L1 = mc->lv[0];
    HIP_OK(hipMemsetAsync(L1->A.p, 0, L1->A.n * sizeof(double), s));
    hipLaunchKernelGGL(k_galerkin0, dim3(c->n_slices), dim3(256), 0, s, gf, mc->v_offset, c->NV, c->n_slices, c->slice_off.p, c->slice_len.p, c->colidx.p, c->perm.p, c->vals.p,
                       L1->A.p);
    if (c->nc > 0) hipLaunchKernelGGL(k_galerkin0_diag, dim3(nblk((gf.N + 1) * (gf.M + 1), 256)), dim3(256), 0, s, gf, mc->v_offset, c->rowpos.p, c->c_diag.p, L1->A.p);
    hipLaunchKernelGGL(k_st_diag_inv, dim3(nblk(L1->n, 256)), dim3(256), 0, s, L1->n, L1->A.p, L1->Dinv.p);
    for (size_t l = 0; l + 1 < mg_levels(c, mc); l++) {
      MgLevel* Lf = mc->lv[l];
      MgLevel* Lc = mc->lv[l + 1];
      HIP_OK(hipMemsetAsync(Lc->A.p, 0, Lc->A.n * sizeof(double), s));
      hipLaunchKernelGGL(k_galerkin_st, dim3(nblk((long)Lf->n * 25, 256)), dim3(256), 0, s, MgGrid{Lf->N, Lf->M}, Lf->A.p, Lc->A.p);
      hipLaunchKernelGGL(k_st_diag_inv, dim3(nblk(Lc->n, 256)), dim3(256), 0, s, Lc->n, Lc->A.p, Lc->Dinv.p);
      // S = P^T A Dinv of the fine level: its first sweep, residual and restriction are one launch.  Both cycle kernels of the level read
      // single-precision copies; S is formed from the ROUNDED A so that the pair stays adjoint up to the rounding of S
      if (Lf->A32.n == 0 && (Lf->A32.alloc(Lf->A.n) | Lf->S32.alloc((size_t)441 * Lc->n))) return tsl_fail("out of device memory (stencil f32 copies)");
      hipLaunchKernelGGL(k_vals_to_f32, dim3(gsz(Lf->A.n)), dim3(256), 0, s, Lf->A.n, Lf->A.p, Lf->A32.p);
      hipLaunchKernelGGL(k_st_build_ra, dim3(nblk((long)Lc->n * 49, 256)), dim3(256), 0, s, MgGrid{Lf->N, Lf->M}, Lf->A32.p, Lf->Dinv.p, Lf->S32.p);
    }
    MgLevel* Ll = mc->lv[mg_levels(c, mc) - 1];
    if (mg_level_dense(c, Ll)) {  // dense inverse of the last level
      const int n3 = 3 * Ll->n;
      if (Ll->Cinv.n == 0) {
        if (Ll->Cinv.alloc((size_t)n3 * n3) | Ll->cbad.alloc(1)) return tsl_fail("out of device memory (coarse inverse)");
      }
      {
        const int ld = (n3 + GJ_B - 1) / GJ_B * GJ_B, nbk = ld / GJ_B;
        if (Ll->gj_ld != ld) {
          if (Ll->gjD.alloc((size_t)ld * ld) | Ll->gjR.alloc((size_t)GJ_B * ld) | Ll->gjC.alloc((size_t)ld * GJ_B) | Ll->gjP.alloc(2 * GJ_B * GJ_B))
            return tsl_fail("out of device memory (coarse inverse workspace)");
          Ll->gj_ld = ld;
        }
        HIP_OK(hipMemsetAsync(Ll->gjD.p, 0, (size_t)ld * ld * sizeof(double), s));
        HIP_OK(hipMemsetAsync(Ll->cbad.p, 0, sizeof(int), s));
        hipLaunchKernelGGL(k_st_dense_build, dim3(nblk((long)Ll->n * 225, 256)), dim3(256), 0, s, MgGrid{Ll->N, Ll->M}, ld, Ll->A.p, Ll->gjD.p);
        hipLaunchKernelGGL(k_st_dense_diag, dim3(nblk(ld, 256)), dim3(256), 0, s, n3, ld, Ll->gjD.p);
        std::vector<double> h_orig;
        if (c->verbose >= 2) {  // diagnostic: keep the matrix to check the inverse on the host
          h_orig.resize((size_t)ld * ld);
          HIP_OK(hipMemcpyAsync(h_orig.data(), Ll->gjD.p, h_orig.size() * sizeof(double), hipMemcpyDeviceToHost, s));
          HIP_OK(hipStreamSynchronize(s));
        }
        double* Pb[2] = {Ll->gjP.p, Ll->gjP.p + GJ_B * GJ_B};  // pivot-block inverses of step k (k & 1) and k + 1
        hipLaunchKernelGGL(k_gj_pivot0, dim3(1), dim3(256), 0, s, ld, Ll->gjD.p, Pb[0], Ll->cbad.p);
        for (int k = 0; k < nbk; k++) {
          hipLaunchKernelGGL(k_gj_panel, dim3(nbk), dim3(256), 0, s, ld, k, Ll->gjD.p, Pb[k & 1], Ll->gjR.p, Ll->gjC.p);
          hipLaunchKernelGGL(k_gj_update, dim3(nbk, nbk), dim3(256), 0, s, ld, k, Ll->gjD.p, Ll->gjR.p, Ll->gjC.p, Pb[k & 1], Pb[(k + 1) & 1], Ll->cbad.p);
        }
        hipLaunchKernelGGL(k_gj_finish, dim3(nblk((long)n3 * n3, 256)), dim3(256), 0, s, n3, ld, Ll->gjD.p, Ll->cbad.p, Ll->Dinv.p, Ll->Cinv.p);
        if (c->verbose >= 2) {
          std::vector<float> h_inv((size_t)n3 * n3);
          int hb = 0;
          HIP_OK(hipMemcpyAsync(h_inv.data(), Ll->Cinv.p, h_inv.size() * sizeof(float), hipMemcpyDeviceToHost, s));
          HIP_OK(hipMemcpyAsync(&hb, Ll->cbad.p, sizeof(int), hipMemcpyDeviceToHost, s));
          HIP_OK(hipStreamSynchronize(s));
          double worst = 0;
          for (int i = 0; i < n3; i++)
            for (int j = 0; j < n3; j++) {
              double acc = 0;
              for (int m = 0; m < n3; m++) acc += (double)h_inv[(size_t)i * n3 + m] * h_orig[(size_t)m * ld + j];
              worst = std::max(worst, fabs(acc - (i == j ? 1.0 : 0.0)));
            }
          fprintf(stderr, "[tsl] dense coarse level %d x %d: n3 %d, max |Cinv A - I| = %.3e, bad pivot flag %d\n", Ll->N + 1, Ll->M + 1, n3, worst, hb);
        }
      }
    }
  }
  // damping factors: omega = 1.5 / lambda_max(D^-1 A) per level, lambda_max from a power iteration
  const double c_om = 1.5, om_max = 0.8;
  if (!c->mg_omega_valid) {
    // lambda_max(D^-1 A) moves little over the Newton iterations of one step and omega = 1.5 / lambda_max keeps a 33 % margin:
    // the power iterations (~220 launches) run at the first assembly of a time / adjoint step only, and again after a breakdown
    c->mg_omega_valid = true;
    const int K = 12;
    {  // level 0: v in v_t2, t in v_t3
      const int NV = c->NV, gb = nblk(NV, 256);
      hipLaunchKernelGGL(k_pi_init, dim3(gb), dim3(256), 0, s, NV, c->v_t2.p);
      for (int k = 0; k < K; k++) {
        mg_spmv0(c, c->v_t2.p, c->v_t3.p);
        hipLaunchKernelGGL(k_pi_apply, dim3(gb), dim3(256), 0, s, NV, c->Dinv.p, c->v_t3.p, c->v_t2.p, c->mg_pi_part.p);
        hipLaunchKernelGGL(k_pi_finish, dim3(1), dim3(256), 0, s, c->mg_pi_part.p, gb, c->mg_pi_norm.p, k, (k == K - 1) ? 1 : 0, c_om, om_max, c->mg_omega0.p);
      }
    }
    for (MgCloth* mc : c->mg)
      for (size_t l = 0; l < mg_levels(c, mc); l++) {
        MgLevel* L = mc->lv[l];
        if (l + 1 == mg_levels(c, mc) && mg_level_dense(c, L)) continue;  // solved exactly: no smoother there
        const int gb = nblk(L->n, 256);
        hipLaunchKernelGGL(k_pi_init, dim3(gb), dim3(256), 0, s, L->n, L->x.p);
        for (int k = 0; k < K; k++) {
          hipLaunchKernelGGL((k_st_spmv5<0>), dim3(nblk(L->n, 64)), dim3(320), 0, s, MgGrid{L->N, L->M}, L->A.p, L->x.p, L->t.p, (const double*)nullptr, (const double*)nullptr,
                             (const double*)nullptr);
          hipLaunchKernelGGL(k_pi_apply, dim3(gb), dim3(256), 0, s, L->n, L->Dinv.p, L->t.p, L->x.p, c->mg_pi_part.p);
          hipLaunchKernelGGL(k_pi_finish, dim3(1), dim3(256), 0, s, c->mg_pi_part.p, gb, c->mg_pi_norm.p, k, (k == K - 1) ? 1 : 0, c_om, om_max, L->omega.p);
        }
      }
  }
  c->mg_ops_valid = true;
  return 0;
}

static constexpr int MG_LAST_SWEEPS = 8;   // damped-Jacobi sweeps on a last level that has no dense inverse

// One V-cycle on stencil level l; returns the buffer (L->x or L->x2) holding the result.  The launch sequence is the same for
// every cycle (required for hipGraph replay).
static double* mg_stencil_cycle(tsl_ctx* c, MgCloth* mc, size_t l) {
  hipStream_t s = c->stream;
  MgLevel* L = mc->lv[l];
  const MgGrid g{L->N, L->M};
  const int gb5 = nblk(L->n, 64);
  double* xa = L->x.p;
  double* xb = L->x2.p;
  if (l + 1 < mg_levels(c, mc)) {
    // x = omega Dinv r and the coarse right-hand side in one launch (k_mg.hpp (1)), the prolongation folded into the post-sweep (2)
    MgLevel* Lc = mc->lv[l + 1];
    hipLaunchKernelGGL(k_st_first_restrict, dim3(nblk(Lc->n, ST_FR_ROWS)), dim3(7 * ST_FR_ROWS), 0, s, g, L->S32.p, L->Dinv.p, L->r.p, L->omega.p, xa, Lc->r.p);
    const double* xc = mg_stencil_cycle(c, mc, l + 1);
    hipLaunchKernelGGL(k_st_prolong_sweep, dim3(gb5), dim3(320), 0, s, g, L->A32.p, xa, xc, xb, L->Dinv.p, L->r.p, L->omega.p);
    return xb;
  }
  if (L->n <= 64 || mg_level_dense(c, L)) {  // the whole last level in one launch
    if (mg_level_dense(c, L) && L->Cinv.n > 0) hipLaunchKernelGGL(k_st_coarse_apply, dim3(nblk(3 * L->n, 8)), dim3(256), 0, s, 3 * L->n, L->Cinv.p, L->r.p, xa);
    else hipLaunchKernelGGL(k_st_coarse, dim3(1), dim3(320), 0, s, g, L->A.p, L->Dinv.p, L->r.p, L->omega.p, MG_LAST_SWEEPS, xa);
    return xa;
  }
  // a last level too large for either: x = omega Dinv r, then xb = xa + omega Dinv (r - A xa) with the roles swapped after each sweep
  hipLaunchKernelGGL(k_mg_jacobi_first, dim3(nblk(L->n, 256)), dim3(256), 0, s, L->n, L->Dinv.p, L->r.p, L->omega.p, xa);
  for (int k = 1; k < MG_LAST_SWEEPS; k++) {
    hipLaunchKernelGGL((k_st_spmv5<1>), dim3(gb5), dim3(320), 0, s, g, L->A.p, xa, xb, L->Dinv.p, L->r.p, L->omega.p);
    std::swap(xa, xb);
  }
  return xa;
}

static bool pcg_fold(tsl_ctx* c) { return mg_active(c) && body_active(c) && c->bd_valid; }

// z = M^-1 r (one V(1,1) cycle); part_rz receives the per-block partials of r.z
static void mg_vcycle(tsl_ctx* c, const double* r, double* z, double* part_rz, bool first_sweep_done = false, bool body_sweep_done = false) {
  hipStream_t s = c->stream;
  const int NV = c->NV, gb = nblk(NV, 256);
  const double* om = c->mg_omega0.p;
  double* t = c->v_mg.p;
  const bool bd = body_active(c) && c->bd_valid;
  if (!first_sweep_done) hipLaunchKernelGGL(k_mg_jacobi_first, dim3(gb), dim3(256), 0, s, NV, c->Dinv.p, r, om, z);
  if (bd && !body_sweep_done) body_apply(c, 0, r, nullptr, z, nullptr, nullptr);
  mg_spmv0(c, z, t);
  for (MgCloth* mc : c->mg) {
    MgLevel* L1 = mc->lv[0];
    hipLaunchKernelGGL(k_mg_restrict0, dim3(nblk(L1->n, 64)), dim3(64), 0, s, MgGrid{mc->N0, mc->M0}, mc->v_offset, c->rowpos.p, r, t, L1->r.p);
    const double* x1 = mg_stencil_cycle(c, mc, 0);
    hipLaunchKernelGGL(k_mg_prolong0_add, dim3(nblk((mc->N0 + 1) * (mc->M0 + 1), 256)), dim3(256), 0, s, MgGrid{mc->N0, mc->M0}, mc->v_offset, c->rowpos.p, x1, z);
  }
  mg_spmv0(c, z, t);
  if (bd) hipLaunchKernelGGL(k_post_smooth, dim3(gb + c->bd_wg), dim3(256), 0, s, c->bd_args, c->bd_Binv.p, gb, NV, c->Dinv.p, r, t, om, z, r, part_rz);
  else hipLaunchKernelGGL(k_mg_jacobi_next, dim3(gb), dim3(256), 0, s, NV, c->Dinv.p, r, t, om, z, r, part_rz);
}


static PcgScal* PSC(tsl_ctx* c) { return (PcgScal*)c->scal.p; }
static PcgScal* HPSC(tsl_ctx* c) { return (PcgScal*)c->h_scal; }

// one PCG iteration = K1 (+ matrix-free contact product) + K2 (+ V-cycle), see k_solver.hpp.  parity selects the p
// ping-pong buffers and the rz history slot; prof (optional) receives per-wave device-clock stamps of K1.
static void launch_pcg_iteration(tsl_ctx* c, int parity, int first, unsigned long long* dprof) {
  hipStream_t s = c->stream;
  const int NV = c->NV, ns = c->n_slices;
  double* p_new = parity ? c->v_t0.p : c->v_p.p;
  const double* p_old = parity ? c->v_p.p : c->v_t0.p;
  // profiling: a chunk launched eagerly for that purpose brackets its first K1 with a hipEvent pair on this stream
  const bool ev = c->ev_sample_next && c->ev_used < c->ev_pool.size();
  c->ev_sample_next = false;
  if (ev) (void)hipEventRecord(c->ev_pool[c->ev_used].first, s);
  hipLaunchKernelGGL((k_pcg_spmv<PCG_WPS, TSL_NT>), dim3(ns), dim3(64 * PCG_WPS), 0, s, NV, ns, c->slice_off.p, c->slice_len.p, c->colidx.p, c->vals.p, c->v_z.p, p_old, p_new,
                     c->v_Ap.p, c->part_rz.p, c->part_rr.p, c->part_pAp.p, PSC(c), parity, first, dprof, contact_rows(c, c->c_H.p));
  if (ev) { (void)hipEventRecord(c->ev_pool[c->ev_used].second, s); c->ev_used++; }
  const bool mg = mg_active(c);
  const bool fold = pcg_fold(c);  // dense-body first sweep inside the update launch
  const int gb = nblk(NV, 256);
  hipLaunchKernelGGL(k_pcg_update, dim3(gb + (fold ? c->bd_wg : 0)), dim3(256), 0, s, NV, p_new, c->v_Ap.p, c->Dinv.p, c->v_x.p, c->v_r.p, c->v_z.p, c->part_pAp.p, c->part_rz.p,
                     c->part_rr.p, PSC(c), parity, (const double*)nullptr, (const double*)nullptr, mg ? 2 : 1, c->mg_omega0.p, gb, c->bd_args, c->bd_Binv.p,
                     fold ? c->bd_rb.p : (double*)nullptr, c->bd_scr_n);
  if (mg) mg_vcycle(c, c->v_r.p, c->v_z.p, c->part_rz.p, true, fold);
  else if (body_active(c) && c->bd_valid) body_apply(c, 0, c->v_r.p, nullptr, c->v_z.p, c->v_r.p, c->part_rz.p + nblk(NV, 256));
}

// Key of the captured launch sequences (PCG chunk, MINRES period): whatever changes a captured launch or a captured pointer.  mg_coarse_exact and
// mg_dense_nodes decide where the hierarchy ends and how its last level is solved, pc_separate which contact blocks the smoother reads, nc the
// contact launches, the dense body inverse and the profile further launches / arguments.
static long solver_graph_key(tsl_ctx* c) {
  const long flags = (mg_active(c) ? 1 : 0) | (c->prof_enable ? 2 : 0) | (c->pc_separate ? 4 : 0) | ((body_active(c) && c->bd_valid) ? 8 : 0) | (c->mg_coarse_exact ? 16 : 0);
  return flags | ((long)(c->mg_dense_nodes & 0xfffff) << 5) | ((long)c->nc << 25);
}

// Chunk of `chunk` (even) iterations with parities 1,0,1,0,... captured once as a hipGraph and replayed: a multigrid-PCG
// iteration is ~20 short kernels.  The first K1 of the chunk stamps
// the device clock into a fixed buffer when profiling is on.
static int pcg_chunk_graph(tsl_ctx* c, int chunk) {
  const long key = (solver_graph_key(c) << 6) | (long)chunk;   // chunk <= 32
  if (c->pcg_graph && c->pcg_graph_key == key) return 0;
  if (c->pcg_graph) { (void)hipGraphExecDestroy(c->pcg_graph); c->pcg_graph = nullptr; }
  hipGraph_t g = nullptr;
  HIP_OK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
  for (int i = 0; i < chunk; i++) launch_pcg_iteration(c, (i & 1) ^ 1, 0, (i == 0 && c->prof_enable) ? c->prof_dev.p : (unsigned long long*)nullptr);
  hipLaunchKernelGGL(k_pcg_check, dim3(1), dim3(256), 0, c->stream, c->part_rr.p, PSC(c));
  HIP_OK(hipStreamEndCapture(c->stream, &g));
  HIP_OK(hipGraphInstantiate(&c->pcg_graph, g, nullptr, nullptr, 0));
  (void)hipGraphDestroy(g);
  c->pcg_graph_key = key;
  return 0;
}

// device-clock span of the stamped K1 launch of the last graph replay (sampled on the host every few chunks)
static int prof_sample_graph(tsl_ctx* c) {
  const size_t nw = c->prof_waves;
  std::vector<unsigned long long> h(2 * nw);
  HIP_OK(hipMemcpyAsync(h.data(), c->prof_dev.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  unsigned long long t0 = ~0ull, t1 = 0;
  for (size_t w = 0; w < nw; w++) { if (h[2 * w + 1] == 0) continue; t0 = std::min(t0, h[2 * w]); t1 = std::max(t1, h[2 * w + 1]); }
  if (t1 > t0) { c->prof_dev_ticks += (double)(t1 - t0); c->prof_dev_n++; }
  return 0;
}

// The forward Hessian is only partially projected by the reference (area and bending blocks go in raw), so a Newton system
// can be indefinite and the preconditioner built from it is then not positive definite either (MINRES breaks down, leaving
// restarted GMRES at ~2.5x the cost per iteration).  Inside tsl_step the state is still at hand: assemble once more with
// EVERY element block projected (spd = 2) into the preconditioner copy and keep the operator untouched -- the same
// separate-preconditioner set-up the adjoint step uses.
static int forward_spd_pc(tsl_ctx* c) {
  if (!c->in_step || c->pc_separate || !c->st_pos || c->mg.empty() || c->mg_enable == 0) return 1;
  hipStream_t s = c->stream;
  if (c->vals_pc.n == 0 && c->vals_pc.alloc(c->vals.n)) return tsl_fail("out of device memory (vals_pc)");
  if (c->nc > 0 && c->c_H_pc.n < c->c_H.n && c->c_H_pc.alloc(c->c_H.n)) return tsl_fail("out of device memory (c_H_pc)");
  // operator -> the "pc" buffers, assemble the SPD variant into the regular ones, then swap the roles back
  std::swap(c->vals.p, c->vals_pc.p);
  if (c->nc > 0) std::swap(c->c_H.p, c->c_H_pc.p);
  const int rc = assemble(c, c->st_pos, c->st_prev, c->st_vel, c->st_ref, 2, nullptr);
  c->mg_omega_valid = false;  // damping factors and dense body blocks of THIS matrix (the lagged ones may be indefinite)
  c->bd_valid = false;
  int rc2 = 0;
  if (!rc) {
    if (body_active(c) && !c->bd_valid) rc2 = body_build_inverse(c);
    if (!rc2) rc2 = mg_setup_operators(c);
  }
  std::swap(c->vals.p, c->vals_pc.p);
  if (c->nc > 0) std::swap(c->c_H.p, c->c_H_pc.p);
  (void)s;
  if (rc || rc2) return -1;
  c->pc_separate = true;
  return 0;
}

// Did the dataflow launches of c's last factorisation lose a flag?  Read when the solve is suspect (not converged) or the test switch "ds_dbg" 21 / 22
// forces the branch (21 as a context without the look-ahead would take it); note = the note of the workgroup that gave up (ds_flow_poll).
// 1: lost (the factors in place are garbage), 0: not, -1: error.  The caller reacts.
static int ds_flow_lost(tsl_ctx* c, bool suspect, int note[8]) {
  const DirectSolver& d = c->ds;
  const bool forced = d.dbg == 21 || d.dbg == 22;
  if (!(suspect || forced) || !d.flow || d.n_flow <= 0) return 0;
  int ab = 0;
  HIP_OK(hipStreamSynchronize(c->stream));
  HIP_OK(hipMemcpy(&ab, d.bad.p + DS_FLOW_ABORT, sizeof(int), hipMemcpyDeviceToHost));
  if (!ab && !forced) return 0;
  for (int k = 0; k < 8; k++) note[k] = 0;
  (void)hipMemcpy(note, d.bad.p + DS_BAD_NOTE, 8 * sizeof(int), hipMemcpyDeviceToHost);
  return 1;
}

// Preconditioned MINRES for symmetric indefinite H with an SPD preconditioner (adjoint systems: un-projected H, preconditioner
// built from the SPD-projected assembly).  Three-term recurrence: one operator product and one preconditioner application
// per iteration like PCG, no basis to orthogonalise against, and for a symmetric H the iterates are those of un-restarted
// GMRES.  H is symmetric only up to the reference's area-Hessian quirk, so the recurrence residual is checked against the true
// residual b - Hx and the recurrence is restarted from it (same rule as the PCG restarts).  The recurrence scalars live on the
// device (MrScal) and six iterations (the period of the buffer rotation) are replayed as one hipGraph; the host reads one
// record per replay.  st->flag = 1 on success, 3 else.
struct MrBufs { double *V[3], *Z[2], *W[3], *x; };

static MrScal* MSC(tsl_ctx* c) { return (MrScal*)c->scal.p; }

static void launch_minres_iteration(tsl_ctx* c, const MrBufs& B, int j) {
  hipStream_t s = c->stream;
  const size_t n3 = 3 * (size_t)c->NV;
  const int gv = gsz(n3);
  double *v_prev = B.V[j % 3], *v_cur = B.V[(j + 1) % 3], *v_next = B.V[(j + 2) % 3];
  double *z_cur = B.Z[j % 2], *z_next = B.Z[(j + 1) % 2];
  double *w_prev = B.W[j % 3], *w_cur = B.W[(j + 1) % 3], *w_next = B.W[(j + 2) % 3];
  MrScal* sc = MSC(c);
  // v_next = H z~_cur with the per-slice partials of z~ . H z~ (no scaling pass, no separate dot launch)
  hipLaunchKernelGGL((k_spmv_mw<4, 1, TSL_NT>), dim3(c->n_slices), dim3(256), 0, s, c->NV, c->n_slices, c->slice_off.p, c->slice_len.p, c->colidx.p, c->vals.p, z_cur, v_next,
                     c->part_pAp.p, &sc->flag, contact_rows(c, c->c_H.p));
  hipLaunchKernelGGL(k_mr_vnext, dim3(gv), dim3(256), 0, s, n3, v_next, v_cur, v_prev, sc, c->part_pAp.p, c->n_slices);
  const bool mg = mg_active(c);
  const bool bd = body_active(c) && c->bd_valid;
  if (mg) mg_vcycle(c, v_next, z_next, c->part_rz.p);  // its last kernel leaves the partials of v_next . z_next in part_rz
  else {
    hipLaunchKernelGGL(k_precond, dim3(nblk(c->NV, 256)), dim3(256), 0, s, c->NV, c->Dinv.p, v_next, z_next);
    if (bd) body_apply(c, 0, v_next, nullptr, z_next, nullptr, nullptr);
    hipLaunchKernelGGL(k_dot, dim3(DOT_BLOCKS), dim3(256), 0, s, n3, z_next, v_next, &sc->g2n, DOT_SCRATCH(c));
  }
  hipLaunchKernelGGL(k_mr_scal, dim3(1), dim3(256), 0, s, sc, mg ? c->part_rz.p : (const double*)nullptr, nblk(c->NV, 256) + (bd ? c->bd_wg : 0));
  hipLaunchKernelGGL(k_mr_wx, dim3(gv), dim3(256), 0, s, n3, z_cur, w_prev, w_cur, w_next, B.x, sc);
  hipLaunchKernelGGL(k_mr_seal, dim3(1), dim3(1), 0, s, sc);
}

static int minres_graph(tsl_ctx* c, const MrBufs& B) {
  const long key = solver_graph_key(c);
  if (c->mr_graph && c->mr_graph_key == key) return 0;
  if (c->mr_graph) { (void)hipGraphExecDestroy(c->mr_graph); c->mr_graph = nullptr; }
  hipGraph_t g = nullptr;
  HIP_OK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
  for (int j = 0; j < 6; j++) launch_minres_iteration(c, B, j);
  HIP_OK(hipStreamEndCapture(c->stream, &g));
  HIP_OK(hipGraphInstantiate(&c->mr_graph, g, nullptr, nullptr, 0));
  (void)hipGraphDestroy(g);
  c->mr_graph_key = key;
  return 0;
}

static int minres(tsl_ctx* c, tsl_solve_stats* st, int cap) {
  hipStream_t s = c->stream;
  const int NV = c->NV;
  const size_t n3 = 3 * (size_t)NV;
  const int gb = nblk(NV, 256), gv = gsz(n3);
  MrBufs B;
  B.V[0] = c->v_t0.p; B.V[1] = c->v_r.p; B.V[2] = c->v_Ap.p;
  B.Z[0] = c->v_z.p; B.Z[1] = c->v_t1.p;
  B.W[0] = c->v_t2.p; B.W[1] = c->v_t3.p; B.W[2] = c->v_p.p;
  B.x = c->v_x.p;
  double* x = B.x;
  const bool mg = mg_active(c);
  if (body_active(c) && !c->bd_valid) TSL_TRY(body_build_inverse(c));
  if (mg && !c->mg_ops_valid) TSL_TRY(mg_setup_operators(c));
  auto precond = [&](const double* in, double* out) {
    if (mg) mg_vcycle(c, in, out, c->part_rz.p);
    else {
      hipLaunchKernelGGL(k_precond, dim3(gb), dim3(256), 0, s, NV, c->Dinv.p, in, out);
      if (body_active(c) && c->bd_valid) body_apply(c, 0, in, nullptr, out, nullptr, nullptr);
    }
  };
  MrScal* d = MSC(c);
  MrScal* h = (MrScal*)c->h_scal;
  auto dot2 = [&](const double* a1, const double* b1, const double* a2, const double* b2, double* o1, double* o2) -> int {
    HIP_OK(hipMemsetAsync(&d->delta, 0, 2 * sizeof(double), s));
    hipLaunchKernelGGL(k_dot, dim3(DOT_BLOCKS), dim3(256), 0, s, n3, a1, b1, &d->delta, DOT_SCRATCH(c));
    if (a2) hipLaunchKernelGGL(k_dot, dim3(DOT_BLOCKS), dim3(256), 0, s, n3, a2, b2, &d->g2n, DOT_SCRATCH(c));
    HIP_OK(hipMemcpyAsync(&h->delta, &d->delta, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    *o1 = h->delta;
    if (o2) *o2 = h->g2n;
    return 0;
  };
  double bb;
  TSL_TRY(dot2(c->v_b.p, c->v_b.p, nullptr, nullptr, &bb, nullptr));
  st->flag = 3;
  if (!(bb > 0)) { st->flag = 1; return 0; }
  const double tol = c->cg_tol * sqrt(bb);
  HIP_OK(hipMemsetAsync(x, 0, n3 * sizeof(double), s));
  HIP_OK(hipMemcpyAsync(B.V[1], c->v_b.p, n3 * sizeof(double), hipMemcpyDeviceToDevice, s));
  double true_prev = 1e300;
  int total = 0;
  for (int cycle = 0; cycle < 40 && total < cap; cycle++) {
    // (re)start from the true residual held in V[1]
    double rr, g2;
    precond(B.V[1], B.Z[0]);
    TSL_TRY(dot2(B.V[1], B.V[1], B.Z[0], B.V[1], &rr, &g2));
    const double rnorm0 = sqrt(rr);
    st->rel_residual = rnorm0 / sqrt(bb);
    if (rnorm0 <= tol) { st->flag = 1; break; }
    if (cycle > 0 && rnorm0 > 0.25 * true_prev && rnorm0 <= 1e2 * tol) { st->flag = 1; st->attained = 1; break; }  // attainable accuracy
    if (cycle > 3 && rnorm0 > 0.9 * true_prev) break;                                            // stagnating: hand over
    true_prev = rnorm0;
    if (!(g2 > 0) || !std::isfinite(g2)) break;  // preconditioner not positive definite
    if (cycle > 0) st->restarts++;
    MrScal hs;
    memset(&hs, 0, sizeof(hs));
    hs.gamma = sqrt(g2); hs.gamma_prev = 1.0; hs.eta = hs.gamma; hs.c_prev = 1.0; hs.c_cur = 1.0;
    hs.thresh_eta = 0.3 * (tol / rnorm0) * hs.gamma;  // the recurrence cycle stops at |eta| <= 0.3 tol: |eta| is the residual in the M^-1 norm, scaled by the start of the cycle; the true residual decides afterwards
    HIP_OK(hipMemcpyAsync(d, &hs, sizeof(MrScal), hipMemcpyHostToDevice, s));
    HIP_OK(hipMemsetAsync(B.V[0], 0, n3 * sizeof(double), s));
    HIP_OK(hipMemsetAsync(B.W[0], 0, n3 * sizeof(double), s));
    HIP_OK(hipMemsetAsync(B.W[1], 0, n3 * sizeof(double), s));
    TSL_TRY(minres_graph(c, B));
    int flag = 0;
    const int base = total;
    while (total < cap) {
      HIP_OK(hipGraphLaunch(c->mr_graph, s));
      HIP_OK(hipMemcpyAsync(h, d, sizeof(MrScal), hipMemcpyDeviceToHost, s));
      HIP_OK(hipStreamSynchronize(s));
      flag = h->flag;
      total = base + h->iters;
      if (flag) break;
    }
    st->iters += h->iters;
    if (c->verbose) fprintf(stderr, "[tsl] MINRES cycle %d: %d iterations from true residual %.3e (tol %.3e), recurrence |eta| %.3e\n", cycle, h->iters, rnorm0, tol, fabs(h->eta));
    // true residual into V[1]
    launch_spmv(c, c->vals.p, x, B.V[2], -1, 0);
    HIP_OK(hipMemcpyAsync(B.V[1], c->v_b.p, n3 * sizeof(double), hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(k_axpby, dim3(gv), dim3(256), 0, s, n3, -1.0, B.V[2], 1.0, B.V[1]);
    if (c->verbose && flag != 2) fprintf(stderr, "[tsl] MINRES stopped: flag %d iters %d gamma %.3e delta %.3e g2n %.3e eta %.3e\n", flag, h->iters, h->gamma, h->delta, h->g2n, h->eta);
    if (flag != 2) {  // breakdown or iteration cap
      double tr;
      TSL_TRY(dot2(B.V[1], B.V[1], nullptr, nullptr, &tr, nullptr));
      st->rel_residual = sqrt(tr / bb);
      if (sqrt(tr) <= tol) st->flag = 1;
      break;
    }
  }
  HIP_OK(hipGetLastError());
  return 0;
}

// Right-preconditioned restarted GMRES(m) on H for indefinite / non-symmetric systems (un-projected adjoint Hessians):
// minimal residual over the Krylov space, so it cannot diverge the way BiCGStab does on strongly indefinite matrices.
// Preconditioner: multigrid V-cycle (+ dense body blocks) when available, else block Jacobi.  Classical Gram-Schmidt applied
// twice with the coefficients kept on the device; one host read (h, h2, |w|^2) per iteration for the Givens rotations.
static int gmres(tsl_ctx* c, tsl_solve_stats* st, int cap, bool direct = false) {
  hipStream_t s = c->stream;
  const int NV = c->NV;
  const size_t n3 = 3 * (size_t)NV;
  const int gb = nblk(NV, 256), gv = gsz(n3);
  // with the factorisation of the operator itself as preconditioner a cycle is a handful of refinement steps
  const int m = (int)std::min<size_t>((size_t)std::max(5, std::min(direct ? std::min(c->gmres_m, 30) : c->gmres_m, 400)), n3);
  if (c->gm_V.n < (size_t)(m + 1) * n3 && c->gm_V.alloc((size_t)(m + 1) * n3)) return tsl_fail("out of device memory (GMRES basis)");
  if (c->gm_h.n < (size_t)(2 * (m + 1) + 2) && c->gm_h.alloc(2 * (size_t)(m + 1) + 2)) return -1;
  double* V = c->gm_V.p;
  double* dh = c->gm_h.p;  // [0, m+1): h ; [m+1, 2m+2): h2 ; [2m+2]: |w|^2
  const int o2 = m + 1, on = 2 * (m + 1);
  double *x = c->v_x.p, *r = c->v_r.p, *w = c->v_Ap.p, *z = c->v_z.p, *u = c->v_t0.p;
  // direct mode keeps the preconditioned basis Z_j = M^-1 V_j (flexible GMRES): the update x += Z y needs no second application
  if (direct && c->gm_Z.n < (size_t)m * n3 && c->gm_Z.alloc((size_t)m * n3)) return tsl_fail("out of device memory (GMRES Z basis)");
  double* Zb = c->gm_Z.p;
  const bool mg = !direct && mg_active(c);
  if (!direct) {
    if (body_active(c) && !c->bd_valid) TSL_TRY(body_build_inverse(c));
    if (mg && !c->mg_ops_valid) TSL_TRY(mg_setup_operators(c));
  }
  auto precond = [&](const double* in, double* out) {
    if (direct) (void)direct_apply(c, in, out);
    else if (mg) mg_vcycle(c, in, out, c->part_rz.p);
    else {
      hipLaunchKernelGGL(k_precond, dim3(gb), dim3(256), 0, s, NV, c->Dinv.p, in, out);
      if (body_active(c) && c->bd_valid) body_apply(c, 0, in, nullptr, out, nullptr, nullptr);
    }
  };
  std::vector<double> hh(2 * (size_t)(m + 1) + 2);
  auto read_h = [&](int cnt) -> int {
    HIP_OK(hipMemcpyAsync(hh.data(), dh, (size_t)cnt * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    return 0;
  };
  auto norm2 = [&](const double* a, double* out) -> int {
    HIP_OK(hipMemsetAsync(dh + on, 0, sizeof(double), s));
    hipLaunchKernelGGL(k_dot, dim3(DOT_BLOCKS), dim3(256), 0, s, n3, a, a, dh + on, DOT_SCRATCH(c));
    HIP_OK(hipMemcpyAsync(out, dh + on, sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    return 0;
  };
  HIP_OK(hipMemsetAsync(x, 0, n3 * sizeof(double), s));
  HIP_OK(hipMemcpyAsync(r, c->v_b.p, n3 * sizeof(double), hipMemcpyDeviceToDevice, s));
  double bb;
  TSL_TRY(norm2(r, &bb));
  if (!(bb > 0)) { st->flag = 1; return 0; }
  const double tol = c->cg_tol * sqrt(bb);
  double beta = sqrt(bb);
  st->flag = 3;
  std::vector<double> H((size_t)(m + 1) * m), cs(m), sn(m), g(m + 1), y(m);
  int total = 0;
  double beta_prev = 1e300;
  for (int cycle = 0; cycle < 1000 && total < cap; cycle++) {
    hipLaunchKernelGGL(k_axpby, dim3(gv), dim3(256), 0, s, n3, 1.0 / beta, r, 0.0, V);
    std::fill(g.begin(), g.end(), 0.0);
    g[0] = beta;
    int j = 0;
    for (; j < m; j++) {
      double* vj1 = V + (size_t)(j + 1) * n3;
      if (direct) z = Zb + (size_t)j * n3;
      precond(V + (size_t)j * n3, z);
      launch_spmv(c, c->vals.p, z, w, -1, 0);
      HIP_OK(hipMemsetAsync(dh, 0, (size_t)(on + 1) * sizeof(double), s));
      hipLaunchKernelGGL(k_multi_dot, dim3(64, j + 1), dim3(256), 0, s, n3, V, n3, w, dh, DOT_SCRATCH(c));
      hipLaunchKernelGGL(k_multi_axpy, dim3(gv), dim3(256), 0, s, n3, V, n3, j + 1, dh, -1.0, w);
      hipLaunchKernelGGL(k_multi_dot, dim3(64, j + 1), dim3(256), 0, s, n3, V, n3, w, dh + o2, DOT_SCRATCH(c));
      hipLaunchKernelGGL(k_multi_axpy, dim3(gv), dim3(256), 0, s, n3, V, n3, j + 1, dh + o2, -1.0, w);
      hipLaunchKernelGGL(k_dot, dim3(DOT_BLOCKS), dim3(256), 0, s, n3, w, w, dh + on, DOT_SCRATCH(c));
      TSL_TRY(read_h(on + 1));
      total++; st->iters++;
      const double hn = sqrt(std::max(hh[on], 0.0));
      double* Hj = &H[(size_t)j * (m + 1)];  // column j
      for (int i = 0; i <= j; i++) Hj[i] = hh[i] + hh[o2 + i];
      Hj[j + 1] = hn;
      for (int i = 0; i < j; i++) {  // previous rotations
        const double t0 = cs[i] * Hj[i] + sn[i] * Hj[i + 1];
        Hj[i + 1] = -sn[i] * Hj[i] + cs[i] * Hj[i + 1];
        Hj[i] = t0;
      }
      const double den = hypot(Hj[j], Hj[j + 1]);
      if (!(den > 0) || !std::isfinite(den)) { j++; break; }
      cs[j] = Hj[j] / den; sn[j] = Hj[j + 1] / den;
      Hj[j] = den; Hj[j + 1] = 0;
      g[j + 1] = -sn[j] * g[j];
      g[j] = cs[j] * g[j];
      st->rel_residual = fabs(g[j + 1]) / sqrt(bb);
      if (direct && c->verbose >= 5) fprintf(stderr, "[tsl]     refinement %d: rel_residual %.2e\n", total, st->rel_residual);
      if (fabs(g[j + 1]) <= (direct ? 1.0 : 0.5) * tol || !(hn > 0)) { j++; break; }   // the true residual is checked below either way
      hipLaunchKernelGGL(k_axpby, dim3(gv), dim3(256), 0, s, n3, 1.0 / hn, w, 0.0, vj1);
    }
    // y = R^-1 g ; x += M^-1 (V y)
    const int k = j;
    for (int i = k - 1; i >= 0; i--) {
      double t0 = g[i];
      for (int l = i + 1; l < k; l++) t0 -= H[(size_t)l * (m + 1) + i] * y[l];
      const double d = H[(size_t)i * (m + 1) + i];
      y[i] = d != 0 ? t0 / d : 0.0;
    }
    HIP_OK(hipMemcpyAsync(dh, y.data(), (size_t)k * sizeof(double), hipMemcpyHostToDevice, s));
    if (direct) hipLaunchKernelGGL(k_multi_axpy, dim3(gv), dim3(256), 0, s, n3, Zb, n3, k, dh, 1.0, x);
    else {
      HIP_OK(hipMemsetAsync(u, 0, n3 * sizeof(double), s));
      hipLaunchKernelGGL(k_multi_axpy, dim3(gv), dim3(256), 0, s, n3, V, n3, k, dh, 1.0, u);
      precond(u, z);
      hipLaunchKernelGGL(k_axpby, dim3(gv), dim3(256), 0, s, n3, 1.0, z, 1.0, x);
    }
    // true residual (and |x| for the backward error of the direct mode) behind ONE host synchronisation, which also covers the
    // upload of y above (the host vector is reused by the next cycle only after it)
    launch_spmv(c, c->vals.p, x, w, -1, 0);
    HIP_OK(hipMemcpyAsync(r, c->v_b.p, n3 * sizeof(double), hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(k_axpby, dim3(gv), dim3(256), 0, s, n3, -1.0, w, 1.0, r);
    double rr, xx = 0.0;
    {
      HIP_OK(hipMemsetAsync(dh + on, 0, 2 * sizeof(double), s));
      hipLaunchKernelGGL(k_dot, dim3(DOT_BLOCKS), dim3(256), 0, s, n3, (const double*)r, (const double*)r, dh + on, DOT_SCRATCH(c));
      if (direct) hipLaunchKernelGGL(k_dot, dim3(DOT_BLOCKS), dim3(256), 0, s, n3, (const double*)x, (const double*)x, dh + on + 1, DOT_SCRATCH(c));
      double two[2];
      HIP_OK(hipMemcpyAsync(two, dh + on, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
      HIP_OK(hipStreamSynchronize(s));
      rr = two[0]; xx = two[1];
    }
    beta = sqrt(rr);
    st->rel_residual = beta / sqrt(bb);
    if (!std::isfinite(beta)) break;
    if (beta <= tol) { st->flag = 1; break; }
    if (direct) {
      // Attainable accuracy of a factorisation-based solve: the reference's spsolve returns a backward-stable solution, i.e. a
      // residual of the order eps |H| |x|, which on the near-singular adjoint operators of a long rollout (|H| |x| / |b| up to
      // 1e9) is ABOVE cg_tol |b|.  When refinement no longer halves the true residual the normwise backward error
      // |b - Hx| / (|H|_inf |x| + |b|) decides: below 1e-12 (a few thousand eps, the n eps growth bound of a pivoted sparse LU in
      // practice) the solution is what a direct solver delivers (reported as attained).
      TSL_TRY(direct_anorm(c));
      st->backward_error = beta / (c->ds.anorm * sqrt(xx) + sqrt(bb));
      if (cycle > 0 && beta > 0.5 * beta_prev && st->backward_error <= 1e-12) { st->flag = 1; st->attained = 1; break; }
      if (cycle >= 8) break;
    } else {
      // attainable accuracy (same rule as the PCG restarts)
      if (cycle > 0 && beta > 0.5 * beta_prev && beta <= 50 * tol) { st->flag = 1; st->attained = 1; break; }
      if (cycle > 20 && beta > 0.9 * beta_prev) break;  // stagnating restarts: hand over to BiCGStab
    }
    beta_prev = beta;
    st->restarts++;
  }
  return 0;
}

// One pass of the refinement below, enqueued on c's stream: r = b - H x with x = v_x, and {r.r, x.x, b.b, max |x_i|} -> h_ir (ONE fused kernel,
// fixed summation order).  The caller synchronises the stream and judges the pass (ir_pass_verdict).
static int ir_pass_enqueue(tsl_ctx* c) {
  hipStream_t s = c->stream;
  const size_t n3 = 3 * (size_t)c->NV;
  const int gv = std::min(gsz(n3), 240);
  if (c->ir_part.n < (size_t)4 * 240 + 8 && c->ir_part.alloc(4 * 240 + 8)) return -1;
  if (c->ir_ticket.n < 2) { if (c->ir_ticket.alloc(2)) return -1; HIP_OK(hipMemsetAsync(c->ir_ticket.p, 0, 2 * sizeof(int), s)); }
  if (c->h_ir == nullptr) HIP_OK(hipHostMalloc((void**)&c->h_ir, 8 * sizeof(double)));
  double* out = c->ir_part.p + 4 * 240;
  launch_spmv(c, c->vals.p, c->v_x.p, c->v_Ap.p, -1, 0);
  hipLaunchKernelGGL(k_ir_resid, dim3(gv), dim3(256), 0, s, n3, (const double*)c->v_b.p, (const double*)c->v_Ap.p, (const double*)c->v_x.p, c->v_r.p, c->ir_part.p, c->ir_ticket.p, out);
  HIP_OK(hipMemcpyAsync(c->h_ir, out, 4 * sizeof(double), hipMemcpyDeviceToHost, s));
  return 0;
}

// The verdict on a pass whose norms are in h_ir: counts it, records its max |x_i| and relative residual, and accepts it (st->flag = 1, returns 1)
// on a zero right-hand side, on |b - Hx| <= cg_tol |b| or -- first pass only -- on the normwise backward-error rule.  0: not accepted, -1: error.
static int ir_pass_verdict(tsl_ctx* c, tsl_solve_stats* st, bool first) {
  DirectSolver& d = c->ds;
  const double rr = c->h_ir[0], xx = c->h_ir[1], bb = c->h_ir[2];
  c->last_xmax = c->h_ir[3]; c->last_xmax_valid = true;   // max |x_i| of the iterate this residual belongs to
  st->iters++;
  if (!(bb > 0)) { st->flag = 1; st->rel_residual = 0; return 1; }   // zero right-hand side: x = 0
  st->rel_residual = sqrt(rr / bb);
  if (c->verbose >= 5) fprintf(stderr, "[tsl]     refinement %d: rel_residual %.2e\n", st->iters, st->rel_residual);
  if (!std::isfinite(rr)) return 0;
  if (rr <= c->cg_tol * c->cg_tol * bb) { st->flag = 1; return 1; }
  // Stop rule of the FIRST pass (round 5): the reference's spsolve (sparse_solver.py:96-103) returns the un-refined answer of a sparse LU,
  // which on the cfg4 operators leaves 5e-11 of |b| (scipy's SuperLU, bench.py cpu_baseline) -- where this LU's first pass lands too (median
  // 4e-11..1e-10, 99 % below 1.5e-9: scripts/probe_berr.py).  cg_tol = 1e-10 cut that distribution in half and sent 45-80 % of the solves
  // through a second application of the factors.  A first pass is now accepted when it is BACKWARD STABLE in the normwise sense xGERFS and the
  // adjoint's attainable-accuracy rule below use -- |b - Hx| / (|H|_inf |x| + |b|) <= "direct_berr" (1e-12, the bound of that rule; measured
  // 1e-17..1e-16) -- AND its forward residual is within "direct_berr_rel_cap" x cg_tol (50: 5e-9).  The componentwise (Oettli-Prager) error of
  // the same passes is 1e-12..2e-11: an LU without row exchanges is not componentwise stable next to contact entries of 1e13, which is what
  // further passes repair and why the forward bound stays as the guard.
  if (first && d.berr_tol > 0 && rr <= d.berr_rel_cap * d.berr_rel_cap * c->cg_tol * c->cg_tol * bb) {
    TSL_TRY(direct_anorm(c));
    const double be = sqrt(rr) / (d.anorm * sqrt(xx) + sqrt(bb));
    d.berr_seen++;
    if (c->verbose >= 5) fprintf(stderr, "[tsl]       normwise backward error %.2e\n", be);
    if (be <= d.berr_tol) {
      st->flag = 1; st->backward_error = be;   // (counted in tsl_direct_counters: berr_accepted, berr_max, berr_rel_max; `attained` keeps its meaning)
      d.berr_accepted++; d.berr_max = std::max(d.berr_max, be); d.berr_rel_max = std::max(d.berr_rel_max, st->rel_residual);
      return 1;
    }
  }
  return 0;
}

// Refinement of the factorised solve (primary path of the direct mode): x = M^-1 b, then x += M^-1 (b - H x) until the true
// residual meets cg_tol -- classic iterative refinement with the multifrontal factors as M^-1.  One application of the factors,
// one operator product, ONE fused kernel (residual + the three norms, fixed summation order) and ONE host synchronisation per
// step; the flexible GMRES above spends 2 products, ~12 vector launches and 3-4 synchronisations on a one-iteration solve and is
// kept for the systems refinement does not contract on (flag stays 3: the caller runs it from scratch).  Same acceptance rules:
// |b - Hx| <= cg_tol |b|, or -- when a step no longer halves the residual -- a normwise backward error below 1e-12 ("attained").
// first_done: the first pass is in place and judged already, its norms in h_ir and its counts in st (scene group: the merged application
// of the factors of every member, group_solve); the refinement goes on from the second pass.
static int direct_refine(tsl_ctx* c, tsl_solve_stats* st, bool first_done = false) {
  hipStream_t s = c->stream;
  const size_t n3 = 3 * (size_t)c->NV;
  double *x = c->v_x.p, *r = c->v_r.p, *z = c->v_z.p;
  st->flag = 3;
  double rr_prev = 1e300;
  for (int it = 0; it < 4; it++) {
    if (it > 0 || !first_done) {
      if (it == 0) TSL_TRY(direct_apply(c, c->v_b.p, x));
      else {
        TSL_TRY(direct_apply(c, r, z));
        hipLaunchKernelGGL(k_axpby, dim3(gsz(n3)), dim3(256), 0, s, n3, 1.0, (const double*)z, 1.0, x);
      }
      TSL_TRY(ir_pass_enqueue(c));
      HIP_OK(hipStreamSynchronize(s));
      const int ok = ir_pass_verdict(c, st, it == 0);
      if (ok) return ok < 0 ? -1 : 0;
    }
    const double rr = c->h_ir[0], xx = c->h_ir[1], bb = c->h_ir[2];
    if (!std::isfinite(rr)) return 0;
    if (it > 0 && rr > 0.25 * rr_prev) {   // no longer contracting: accepted at the accuracy a backward-stable direct solve attains, or handed to GMRES
      TSL_TRY(direct_anorm(c));
      st->backward_error = sqrt(rr) / (c->ds.anorm * sqrt(xx) + sqrt(bb));
      if (st->backward_error <= 1e-12) { st->flag = 1; st->attained = 1; }
      return 0;
    }
    rr_prev = rr;
  }
  return 0;
}

// Block-Jacobi BiCGStab on H (used when PCG breaks down: un-projected adjoint Hessians can be indefinite)
static int bicgstab(tsl_ctx* c, tsl_solve_stats* st, int cap) {
  hipStream_t s = c->stream;
  const int NV = c->NV;
  const size_t n3 = 3 * (size_t)NV;
  const int gb = nblk(NV, 256), gv = gsz(n3);
  double *x = c->v_x.p, *r = c->v_r.p, *r0 = c->v_t0.p, *p = c->v_p.p, *v = c->v_Ap.p, *sv = c->v_t1.p, *t = c->v_t2.p, *ph = c->v_z.p, *sh = c->v_t3.p;
  HIP_OK(hipMemsetAsync(x, 0, n3 * sizeof(double), s));
  HIP_OK(hipMemcpyAsync(r, c->v_b.p, n3 * sizeof(double), hipMemcpyDeviceToDevice, s));
  HIP_OK(hipMemcpyAsync(r0, c->v_b.p, n3 * sizeof(double), hipMemcpyDeviceToDevice, s));
  HIP_OK(hipMemsetAsync(p, 0, n3 * sizeof(double), s));
  HIP_OK(hipMemsetAsync(v, 0, n3 * sizeof(double), s));
  CgScal* d = SC(c);
  CgScal* h = HSC(c);
  auto dots = [&](const double* a1, const double* b1, const double* a2, const double* b2, double* o1, double* o2) -> int {
    HIP_OK(hipMemsetAsync(&d->aux[0], 0, 2 * sizeof(double), s));
    hipLaunchKernelGGL(k_dot, dim3(DOT_BLOCKS), dim3(256), 0, s, n3, a1, b1, &d->aux[0], DOT_SCRATCH(c));
    if (a2) hipLaunchKernelGGL(k_dot, dim3(DOT_BLOCKS), dim3(256), 0, s, n3, a2, b2, &d->aux[1], DOT_SCRATCH(c));
    HIP_OK(hipMemcpyAsync(&h->aux[0], &d->aux[0], 2 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    *o1 = h->aux[0];
    if (o2) *o2 = h->aux[1];
    return 0;
  };
  const bool mg = mg_active(c);
  if (body_active(c) && !c->bd_valid) TSL_TRY(body_build_inverse(c));
  if (mg && !c->mg_ops_valid) TSL_TRY(mg_setup_operators(c));
  auto precond = [&](const double* in, double* out) {  // right preconditioner: multigrid V-cycle when available, else block Jacobi
    if (mg) mg_vcycle(c, in, out, c->part_rz.p);
    else {
      hipLaunchKernelGGL(k_precond, dim3(gb), dim3(256), 0, s, NV, c->Dinv.p, in, out);
      if (body_active(c) && c->bd_valid) body_apply(c, 0, in, nullptr, out, nullptr, nullptr);
    }
  };
  double bb;
  TSL_TRY(dots(c->v_b.p, c->v_b.p, nullptr, nullptr, &bb, nullptr));
  double rho = 1, alpha = 1, omega = 1;
  const double tol2 = c->cg_tol * c->cg_tol * bb;
  st->flag = 3;
  int restarts_left = 50;
  auto restart = [&]() -> int {  // breakdown (rho or omega vanished): restart the recurrence from the current residual
    HIP_OK(hipMemcpyAsync(r0, r, n3 * sizeof(double), hipMemcpyDeviceToDevice, s));
    HIP_OK(hipMemsetAsync(p, 0, n3 * sizeof(double), s));
    HIP_OK(hipMemsetAsync(v, 0, n3 * sizeof(double), s));
    rho = alpha = omega = 1;
    st->restarts++;
    return 0;
  };
  for (int it = 0; it < cap; it++) {
    double rho_new;
    TSL_TRY(dots(r0, r, nullptr, nullptr, &rho_new, nullptr));
    if (fabs(rho_new) < 1e-300 || omega == 0 || !std::isfinite(rho_new)) {
      if (restarts_left-- <= 0 || !std::isfinite(rho_new)) break;
      TSL_TRY(restart());
      TSL_TRY(dots(r0, r, nullptr, nullptr, &rho_new, nullptr));
      if (!(fabs(rho_new) > 0)) break;
    }
    const double beta = (rho_new / rho) * (alpha / omega);
    rho = rho_new;
    // p = r + beta (p - omega v)
    hipLaunchKernelGGL(k_axpby, dim3(gv), dim3(256), 0, s, n3, -omega, v, 1.0, p);
    hipLaunchKernelGGL(k_axpby, dim3(gv), dim3(256), 0, s, n3, 1.0, r, beta, p);
    precond(p, ph);
    launch_spmv(c, c->vals.p, ph, v, -1, 0);
    double r0v;
    TSL_TRY(dots(r0, v, nullptr, nullptr, &r0v, nullptr));
    if (r0v == 0) { if (restarts_left-- <= 0) break; TSL_TRY(restart()); continue; }
    alpha = rho / r0v;
    // s = r - alpha v
    HIP_OK(hipMemcpyAsync(sv, r, n3 * sizeof(double), hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(k_axpby, dim3(gv), dim3(256), 0, s, n3, -alpha, v, 1.0, sv);
    precond(sv, sh);
    launch_spmv(c, c->vals.p, sh, t, -1, 0);
    double tt, ts;
    TSL_TRY(dots(t, t, t, sv, &tt, &ts));
    omega = tt > 0 ? ts / tt : 0;
    hipLaunchKernelGGL(k_axpby, dim3(gv), dim3(256), 0, s, n3, alpha, ph, 1.0, x);
    hipLaunchKernelGGL(k_axpby, dim3(gv), dim3(256), 0, s, n3, omega, sh, 1.0, x);
    HIP_OK(hipMemcpyAsync(r, sv, n3 * sizeof(double), hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(k_axpby, dim3(gv), dim3(256), 0, s, n3, -omega, t, 1.0, r);
    st->iters += 2;
    double rr;
    TSL_TRY(dots(r, r, nullptr, nullptr, &rr, nullptr));
    st->rel_residual = sqrt(rr / bb);
    if (rr <= 0.25 * tol2) {
      // verify with the true residual
      launch_spmv(c, c->vals.p, x, t, -1, 0);
      HIP_OK(hipMemcpyAsync(sv, c->v_b.p, n3 * sizeof(double), hipMemcpyDeviceToDevice, s));
      hipLaunchKernelGGL(k_axpby, dim3(gv), dim3(256), 0, s, n3, -1.0, t, 1.0, sv);
      double tr;
      TSL_TRY(dots(sv, sv, nullptr, nullptr, &tr, nullptr));
      st->rel_residual = sqrt(tr / bb);
      if (tr <= 100 * tol2) { st->flag = 1; break; }
      HIP_OK(hipMemcpyAsync(r, sv, n3 * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------ linear solve
// Right-hand side in v_b (permuted), result in v_x (permuted).  solve_perm sends a solve to the factorisation (solve_direct) or to the iterative
// hierarchy (hierarchy_solve: pcg_restarts, then hierarchy_fallback).  solve_direct runs the hierarchy as its probe and as its fallback; every
// run of the hierarchy is told its iteration cap and its mode by the caller.
enum HierMode { HIER_FULL, HIER_PROBE };   // HIER_PROBE: a PCG that does not converge within the cap ends the run with flag 3 (no fallback solvers)
static int hierarchy_solve(tsl_ctx* c, tsl_solve_stats* st, int cap, HierMode mode);

static void solve_stats_reset(tsl_ctx* c, tsl_solve_stats* st) {
  st->iters = 0; st->restarts = 0; st->flag = 0; st->rel_residual = 0; st->method = 0; st->attained = 0; st->backward_error = 0;
  c->last_xmax_valid = false;
}

struct PcgOutcome { bool need_fallback = false, indefinite = false; };

// Multigrid- or block-Jacobi-preconditioned CG, restarted from the true residual (at most 20 times); st->iters counts at most `cap` iterations
// (to the chunk).  out->need_fallback: not converged; out->indefinite: the recurrence met a direction of non-positive curvature.
// The start of a PCG run in three parts, shared by pcg_restarts and tsl_pcg_trace (op_test_api.hpp), so that the traced iterations start exactly
// where the solver's do.  pcg_begin: x = 0, |b|^2 (returned; 0: nothing to solve), the set-up of the preconditioners.
static int pcg_begin(tsl_ctx* c, double* bb_out) {
  hipStream_t s = c->stream;
  const size_t n3 = 3 * (size_t)c->NV;
  *bb_out = 0;
  TSL_TRY(block_jacobi_ensure(c));   // (skipped by an assembly that expected the factorisation to take this solve)
  HIP_OK(hipMemsetAsync(c->v_x.p, 0, n3 * sizeof(double), s));
  HIP_OK(hipMemsetAsync(c->scal.p, 0, sizeof(SolverScalars), s));
  hipLaunchKernelGGL(k_dot, dim3(DOT_BLOCKS), dim3(256), 0, s, n3, c->v_b.p, c->v_b.p, &SC(c)->bb, DOT_SCRATCH(c));
  TSL_TRY(read_scal(c));
  const double bb = HSC(c)->bb;
  if (!(bb > 0)) return 0;  // zero rhs -> x = 0
  if (body_active(c) && !c->bd_valid) TSL_TRY(body_build_inverse(c));
  *bb_out = bb;
  return 0;
}
static int pcg_n_rz(tsl_ctx* c) { return nblk(c->NV, 256) + ((body_active(c) && c->bd_valid) ? c->bd_wg : 0); }
// pcg_start_residual: the scalar record of a (re)start, the true residual r = b - H x (restart: x is not zero), z = Dinv r, the partials of r.r and their sum
static int pcg_start_residual(tsl_ctx* c, double bb, double thresh2, bool restart) {
  hipStream_t s = c->stream;
  const int NV = c->NV, gb = nblk(NV, 256);
  PcgScal hs;
  memset(&hs, 0, sizeof(hs));
  hs.bb = bb; hs.thresh2 = thresh2; hs.n_part1 = c->n_slices; hs.n_part2 = pcg_n_rz(c);
  HIP_OK(hipMemcpyAsync(c->scal.p, &hs, sizeof(PcgScal), hipMemcpyHostToDevice, s));
  if (restart) launch_spmv(c, c->vals.p, c->v_x.p, c->v_Ap.p, -1, 0);
  // true residual, z = M^-1 r, partial r.z / r.r
  hipLaunchKernelGGL(k_pcg_update, dim3(gb + (pcg_fold(c) ? c->bd_wg : 0)), dim3(256), 0, s, NV, (const double*)nullptr, (const double*)nullptr, c->Dinv.p, c->v_x.p, c->v_r.p,
                     c->v_z.p, c->part_pAp.p, c->part_rz.p, c->part_rr.p, PSC(c), 0, c->v_b.p, restart ? c->v_Ap.p : (const double*)nullptr, mg_active(c) ? 0 : 1,
                     (const double*)nullptr, gb, c->bd_args, c->bd_Binv.p, pcg_fold(c) ? c->bd_rb.p : (double*)nullptr, c->bd_scr_n);
  hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, s, c->part_rr.p, gb, &PSC(c)->rr_last);
  return 0;
}
// pcg_start_precond: the rest of z = M^-1 r behind it (the cycle, or the dense body blocks), the sum of the r.z partials
static int pcg_start_precond(tsl_ctx* c) {
  hipStream_t s = c->stream;
  const int gb = nblk(c->NV, 256);
  if (mg_active(c)) {
    if (!c->mg_ops_valid) TSL_TRY(mg_setup_operators(c));
    mg_vcycle(c, c->v_r.p, c->v_z.p, c->part_rz.p);
  } else if (body_active(c) && c->bd_valid) body_apply(c, 0, c->v_r.p, nullptr, c->v_z.p, c->v_r.p, c->part_rz.p + gb);
  hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, s, c->part_rz.p, pcg_n_rz(c), &PSC(c)->rz_last);
  return 0;
}
// iterations per graph replay / host convergence read.  With multigrid: eight on long solves (the previous time step needed more than 150 per
// solve: cfg4 1.56 -> 1.53 s per step), four otherwise (the idle launches after convergence cost drape 4 % with eight).  Block-Jacobi PCG: 32.
static int pcg_chunk(tsl_ctx* c) { return mg_active(c) ? (c->last_step_iters_per_solve > 150.0 ? 8 : 4) : 32; }

static int pcg_restarts(tsl_ctx* c, tsl_solve_stats* st, int cap, PcgOutcome* out) {
  hipStream_t s = c->stream;
  double bb = 0;
  TSL_TRY(pcg_begin(c, &bb));
  if (!(bb > 0)) return 0;  // zero rhs -> x = 0
  const double tol2 = c->cg_tol * c->cg_tol * bb;
  int total_it = 0;
  double rr_prev_outer = 1e300;
  for (int outer = 0; outer < 20; outer++) {
    TSL_TRY(pcg_start_residual(c, bb, 0.25 * tol2, outer > 0));
    if (outer > 0) {  // verification of a converged recurrence: the true residual decides before a V-cycle is spent on it
      TSL_TRY(read_scal(c));
      const double rr1 = HPSC(c)->rr_last;
      st->rel_residual = sqrt(rr1 / bb);
      if (rr1 <= tol2) { out->need_fallback = false; break; }
      // attainable accuracy: when a restart no longer halves the true residual the solve has reached what fp64 allows for
      // this conditioning (a direct solver has the same backward error); accept if within 1e2 of the requested tolerance (reported: attained)
      if (rr1 > 0.25 * rr_prev_outer && rr1 <= 1e4 * tol2) { out->need_fallback = false; st->attained = 1; break; }
    }
    TSL_TRY(pcg_start_precond(c));
    TSL_TRY(read_scal(c));
    const double rr0 = HPSC(c)->rr_last;
    st->rel_residual = sqrt(rr0 / bb);
    if (rr0 <= tol2) { out->need_fallback = false; break; }
    rr_prev_outer = rr0;
    if (!(HPSC(c)->rz_last > 0)) { out->need_fallback = true; break; }
    if (outer > 0) st->restarts++;
    out->need_fallback = true;
    int flag = 0, it = 0;
    const auto tm0 = std::chrono::steady_clock::now();
    // iteration 0 (beta = 0) eagerly, then graph replays of `chunk` iterations (parities 1,0,...)
    launch_pcg_iteration(c, 0, 1, nullptr);
    it++; total_it++; c->prof_launches++;
    const int chunk = pcg_chunk(c);
    TSL_TRY(pcg_chunk_graph(c, chunk));
    int n_chunks = 0;
    // (a second chunk kept in flight behind the one whose convergence record the host waits for was measured and dropped: the time per iteration
    // does not change -- the gaps are between dependent kernels inside the graph, not host round trips -- and the idle chunk cost ~0.2 ms per solve.)
    // A chunk whose device-clock stamps are sampled for the profile gets no successor until read.
    int inflight = 0, head = 0;
    bool sampled[2] = {false, false};
    auto launch_chunk = [&]() -> int {
      const int sl = (head + inflight) & 1;
      // every 32nd chunk of a profiled run is launched kernel by kernel so that one K1 can be timed with hipEvents
      const bool ev_chunk = c->prof_enable && (c->prof_chunks++ % 32 == 16);
      if (!ev_chunk) HIP_OK(hipGraphLaunch(c->pcg_graph, s));
      else {
        c->ev_sample_next = ev_chunk;
        for (int i = 0; i < chunk; i++) launch_pcg_iteration(c, (i & 1) ^ 1, 0, nullptr);
        hipLaunchKernelGGL(k_pcg_check, dim3(1), dim3(256), 0, s, c->part_rr.p, PSC(c));
      }
      HIP_OK(hipMemcpyAsync(&c->h_scal2[sl], c->scal.p, sizeof(CgScal), hipMemcpyDeviceToHost, s));
      HIP_OK(hipEventRecord(c->rb_event[sl], s));
      sampled[sl] = !ev_chunk && c->prof_enable && (n_chunks++ % 8 == 0);
      inflight++; it += chunk; total_it += chunk; c->prof_launches += chunk;
      return 0;
    };
    while (true) {
      while (inflight < 1 && total_it < cap && !(inflight == 1 && sampled[head])) TSL_TRY(launch_chunk());
      if (inflight == 0) break;  // iteration cap
      HIP_OK(hipEventSynchronize(c->rb_event[head]));
      if (sampled[head]) TSL_TRY(prof_sample_graph(c));
      memcpy(c->h_scal, &c->h_scal2[head], sizeof(CgScal));
      inflight--; head ^= 1;
      flag = HPSC(c)->flag;
      if (flag) break;
    }
    if (inflight) HIP_OK(hipStreamSynchronize(s));
    if (c->prof_enable) prof_collect(c);
    c->tm_loop += std::chrono::duration<double>(std::chrono::steady_clock::now() - tm0).count();
    if (flag) total_it = total_it - it + HPSC(c)->iters;  // iterations actually executed before the kernels went idle
    if (flag == 1) { out->indefinite = true; c->mg_omega_valid = false; }
    if (flag != 2) break;  // breakdown or iteration cap
  }
  st->iters = total_it;
  return 0;
}

// What follows a PCG that did not converge: plain block-Jacobi PCG where the multigrid-PCG stalled; else (indefinite operator, or block-Jacobi PCG
// failed too) MINRES -- behind a preconditioner rebuilt from the fully projected assembly if the operator is indefinite --, GMRES, BiCGStab.
static int hierarchy_fallback(tsl_ctx* c, tsl_solve_stats* st, int cap, bool indefinite) {
  if (mg_active(c) && !indefinite) {
    // multigrid-PCG stalled: retry with plain block-Jacobi PCG (an indefinite H goes straight to MINRES)
    Suspend no_mg(c->mg_suspended);
    tsl_solve_stats st2;
    const int rc = hierarchy_solve(c, &st2, cap, HIER_FULL);
    st->iters += st2.iters; st->restarts += st2.restarts + 1; st->flag = st2.flag == 0 ? 1 : st2.flag; st->rel_residual = st2.rel_residual; st->method = st2.method; st->attained = st2.attained;
    return rc;
  }
  if (c->verbose) fprintf(stderr, "[tsl] PCG gave up: iters %d restarts %d rel_residual %.2e indefinite %d\n", st->iters, st->restarts, st->rel_residual, (int)indefinite);
  if (indefinite) {
    const int rcp = forward_spd_pc(c);
    if (rcp < 0) return -1;
    if (c->verbose && rcp == 0) fprintf(stderr, "[tsl] forward system indefinite: preconditioner rebuilt from the fully projected assembly\n");
  }
  {  // symmetric indefinite: short recurrences
    tsl_solve_stats st2 = *st;
    TSL_TRY(minres(c, &st2, cap));
    if (c->verbose) fprintf(stderr, "[tsl] MINRES: flag %d iters %d restarts %d rel_residual %.2e\n", st2.flag, st2.iters - st->iters, st2.restarts, st2.rel_residual);
    st->iters = st2.iters; st->restarts = st2.restarts; st->rel_residual = st2.rel_residual; st->attained = st2.attained;
    if (st2.flag == 1) { st->flag = 1; st->method = 1; return 0; }
  }
  const int it0 = st->iters;
  TSL_TRY(gmres(c, st, cap));
  if (c->verbose) fprintf(stderr, "[tsl] GMRES: flag %d iters %d rel_residual %.2e\n", st->flag, st->iters - it0, st->rel_residual);
  if (st->flag == 1) { st->method = 2; return 0; }
  st->method = 3;
  return bicgstab(c, st, cap);  // last resort
}

// One run of the iterative hierarchy with at most `cap` iterations per solver.  flag 0: PCG converged, 1: a fallback solver did, 3: nothing did.
static int hierarchy_solve(tsl_ctx* c, tsl_solve_stats* st, int cap, HierMode mode) {
  solve_stats_reset(c, st);
  PcgOutcome pcg;
  TSL_TRY(pcg_restarts(c, st, cap, &pcg));
  if (!pcg.need_fallback) { st->flag = 0; return 0; }
  if (mode == HIER_PROBE) { st->flag = 3; return 0; }   // probe of the iterative hierarchy failed: the caller factorises
  return hierarchy_fallback(c, st, cap, pcg.indefinite);
}

// Primary path on refined cloths: multifrontal LU of the operator (like the reference's spsolve) + GMRES refinement against the operator product;
// the iterative hierarchy only runs as the probe of the automatic mode, or if the factorisation fails.  While it does, ds_suspended is set:
// direct_takes_solve must answer "no" to the assembly nested in forward_spd_pc, which has to form the block-Jacobi inverse and the contact diagonal.
// first (scene group): the first pass of the factorised solve is in place and was not accepted (ir_pass_verdict); its statistics -- the solve
// goes on from the second pass, as direct_refine would after its own first pass.
static int solve_direct(tsl_ctx* c, tsl_solve_stats* st, const tsl_solve_stats* first) {
  solve_stats_reset(c, st);
  DirectSolver& d = c->ds;
  // "direct" = -1 (auto): easy systems stay with the iterative hierarchy -- the contact-free 224 x 224 drape needs 26 multigrid-PCG
  // iterations per solve (46 ms per step) against one 6 ms factorisation per solve (86 ms per step).  A solve first probes the
  // hierarchy with a cap of `probe_cap` iterations (the cost of one factorisation); the first failure marks the scene hard and
  // the following `probe_every` time steps go straight to the factorisation.
  // Scenes with FEM bodies or active contacts skip the probe (round 4): it never succeeded on them (cfg3 / cfg4: 60 wasted iterations every
  // 16 steps), and the hierarchy's f64-atomic reductions are the one part of the step that is not bit-reproducible.
  if (!first && d.enable < 0 && !d.hard && c->n_tet == 0 && c->nc == 0) {
    tsl_solve_stats s2;
    int rc;
    { Suspend hierarchy_runs(c->ds_suspended); rc = hierarchy_solve(c, &s2, std::min(c->cg_maxit, d.probe_cap), HIER_PROBE); }
    if (rc) return rc;
    if (s2.flag == 0) { *st = s2; return 0; }
    d.hard = true; d.hard_steps = 0;
    st->iters = s2.iters;   // counted with the solve that follows
  }
  tsl_solve_stats sd = first ? *first : *st;
  // Set-up failures of the direct path (arena or GMRES-basis allocation, an inconsistent plan): with "direct" = 1 they are errors;
  // in the automatic mode the solve falls through to the iterative hierarchy, which needs none of that memory, and after three
  // such failures the context stops trying ("direct" = 0).
  auto direct_try = [&]() -> int {
    if (!d.numeric_valid) {
      TSL_TRY(direct_plan(c));
      TSL_TRY(direct_factor(c, -1, nullptr, c->v_b.p, c->v_x.p));   // (the first pass of direct_refine applies the factors to v_b -> v_x)
    }
    // plain refinement first; systems it does not settle go through the flexible GMRES from scratch
    int rc_g = direct_refine(c, &sd, first != nullptr);
    if (rc_g == 0 && sd.flag != 1) { const int it0 = sd.iters; sd = *st; c->last_xmax_valid = false; rc_g = gmres(c, &sd, c->cg_maxit, true); sd.iters += it0; }
    if (rc_g) return -1;
    int note[8];
    const int lost = ds_flow_lost(c, sd.flag != 1, note);
    if (lost < 0) return -1;
    if (lost) {   // a dataflow launch that lost a flag leaves garbage factors: say so, go back to the launch-per-block-step path
      // The first loss of a context that runs the look-ahead takes the LOOK-AHEAD away (the one known cause inside a process is side-stream work arriving while a launch is
      // still being dispatched) and keeps the dataflow path; a loss without it -- or a second one -- takes the dataflow path.  Either way this system is
      // refactorised on the launch-per-block-step path.
      const bool blame_la = (d.lookahead & 1) != 0 && d.n_flow_abort == 0 && d.dbg != 21;
      fprintf(stderr, "[tsl] k_ds_gj_flow: a workgroup waited in vain for a flag (launch not resident as a whole?): %s disabled for this context, refactorising "
              "(workgroup %d of %d gave up; %d of the %d workgroups of the factorisation's dataflow launches had started; flag value %d, epoch %d)\n",
              blame_la ? "\"direct_lookahead\"" : "\"direct_flow\"", note[2], note[1], note[0], d.flow_wgs_last, note[3], note[4]);
      const int flow_keep = d.flow;
      d.flow = 0; d.n_flow_abort++;
      if (blame_la) d.lookahead = 0;
      d.numeric_valid = false; d.have_factor = false;   // the factors in place are garbage: direct_factor must not return early
      if (d.prezero_pending) { HIP_OK(hipStreamWaitEvent(c->stream, d.ev_zero, 0)); d.prezero_pending = false; }
      TSL_TRY(direct_factor(c));
      if (blame_la) d.flow = flow_keep;
      sd = *st; c->last_xmax_valid = false;
      TSL_TRY(direct_refine(c, &sd));
      if (sd.flag != 1) { const int it0 = sd.iters; sd = *st; c->last_xmax_valid = false; TSL_TRY(gmres(c, &sd, c->cg_maxit, true)); sd.iters += it0; }
    }
    return 0;
  };
  if (direct_try() != 0) {
    if (d.enable == 1) return -1;
    (void)hipGetLastError();   // an out-of-memory allocation leaves a sticky-looking but recoverable error code
    d.numeric_valid = false; d.have_factor = false; d.plan_valid = false;
    fprintf(stderr, "[tsl] direct solver set-up failed (%s): this solve runs on the iterative hierarchy%s\n", tsl_last_error(),
            ++d.n_setup_fail >= 3 ? "; direct path disabled for this context" : "");
    if (d.n_setup_fail >= 3) d.enable = 0;
    Suspend hierarchy_runs(c->ds_suspended);
    const int rc = hierarchy_solve(c, st, c->cg_maxit, HIER_FULL);
    if (rc == 0 && st->flag == 0) st->flag = 1;   // reported as a fallback
    return rc;
  }
  if (sd.flag == 1) { *st = sd; st->flag = 0; st->method = 4; return 0; }
  if (c->verbose) {
    int nb[4] = {0, 0, 0, 0};
    (void)hipMemcpy(nb, d.bad.p, sizeof(nb), hipMemcpyDeviceToHost);
    fprintf(stderr, "[tsl] direct factorisation + GMRES did not converge (rel_residual %.2e, backward error %.2e after %d iterations, perturbed pivots %d / %d / %d in fronts of <= 128 / <= 512 / more pivots, nc %d): iterative fallback\n",
            sd.rel_residual, sd.backward_error, sd.iters, nb[1], nb[2], nb[3], c->nc);
    if (c->verbose > 1) {
      std::vector<int> lg(DS_BAD_NOTE);
      (void)hipMemcpy(lg.data(), d.bad.p, lg.size() * sizeof(int), hipMemcpyDeviceToHost);
      const int nl = std::min(lg[4], DS_BADLOG);
      static int n_dump = 0;
      if (const char* dir = getenv("TSL_DUMP_DIR")) if (nl > 0 && n_dump < 3) {
        char path[512];
        snprintf(path, sizeof(path), "%s/front_%d.bin", dir, n_dump++);
        d.numeric_valid = false;
        TSL_TRY(direct_factor(c, lg[8] >> 6, path));
      }
      for (int i = 0; i < nl; i++) {
        const int* L = &lg[8 + 4 * i];
        const int sn = L[0] >> 6, kt = L[0] & 63;
        const DsFrontDesc& f = d.plan.fr[sn];
        float am; memcpy(&am, L + 3, 4);
        const unsigned mask = (unsigned)L[1];
        const int first = __builtin_ctz(mask | 0x80000000u), row = kt * DS_T + first;
        const int vtx = row < f.p ? d.plan.vtx[f.vtx_off + row / 3] : -1;
        fprintf(stderr, "[tsl]   perturbed pivots: front %d (level %d, p %d, b %d, own verts %d) tile %d rows mask %08x, first row %d (vertex %d dof %d%s), tile max %.3e\n",
                sn, d.plan.sym.level[sn], f.p, f.b, f.nv_own, kt, mask, row, vtx, row % 3, vtx >= 0 && d.plan.sym.body_of[vtx] >= 0 ? ", body" : "", am);
      }
    }
  }
  // Where the refined factorisation stalls, the iterative hierarchy does not do better (it needs 1e4..1e5 iterations on the
  // systems the factorisation is for, and the stalls seen are operators with entries of 1e15 beside 1e3 -- an element of a pad
  // crushed flat late in a rollout): an answer within 1e-3 is returned as it is, flagged not converged; only a broken
  // factorisation (residual above that) is worth a bounded attempt of the hierarchy.
  if (sd.rel_residual <= 1e-3) { *st = sd; st->flag = 3; st->method = 4; return 0; }
  tsl_solve_stats s2;
  int rc;
  {
    Suspend hierarchy_runs(c->ds_suspended);
    HIP_OK(hipMemcpyAsync(c->v_t4.p, c->v_x.p, 3 * (size_t)c->NV * sizeof(double), hipMemcpyDeviceToDevice, c->stream));  // the refined direct solution
    rc = hierarchy_solve(c, &s2, std::min(c->cg_maxit, d.fallback_cap), HIER_FULL);
  }
  // keep the better of the two answers, flagged as not converged.  A non-finite residual never wins: a factorisation that produced
  // Inf / NaN (element entries of 1e15 on a crushed pad) must not overwrite a finite iterate, and two non-finite answers are an error.
  const bool sd_ok = std::isfinite(sd.rel_residual), s2_ok = rc == 0 && std::isfinite(s2.rel_residual);
  if (rc == 0 && s2.flag == 3 && !sd_ok && !s2_ok) return tsl_fail("linear solve: factorisation and iterative fallback both ended with a non-finite residual");
  if (rc == 0 && s2.flag == 3 && sd_ok && (!s2_ok || !(s2.rel_residual < sd.rel_residual))) {
    HIP_OK(hipMemcpyAsync(c->v_x.p, c->v_t4.p, 3 * (size_t)c->NV * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    *st = sd; st->iters = sd.iters + s2.iters; st->flag = 3; st->method = 4;
    return 0;
  }
  st->iters = sd.iters + s2.iters; st->restarts = s2.restarts + 1; st->rel_residual = s2.rel_residual; st->method = s2.method; st->attained = s2.attained;
  st->flag = s2.flag == 0 ? 1 : s2.flag;
  return rc;
}

static int solve_perm(tsl_ctx* c, tsl_solve_stats* st, const tsl_solve_stats* first = nullptr) {
  return direct_enabled(c) ? solve_direct(c, st, first) : hierarchy_solve(c, st, c->cg_maxit, HIER_FULL);
}

static int solve_orig(tsl_ctx* c, const double* rhs, double* x, tsl_solve_stats* st) {
  hipStream_t s = c->stream;
  const int gb = nblk(c->NV, 256);
  hipLaunchKernelGGL(k_gather_perm, dim3(gb), dim3(256), 0, s, c->NV, c->perm.p, rhs, c->v_b.p);
  tsl_solve_stats local;
  if (!st) st = &local;
  TSL_TRY(solve_perm(c, st));
  hipLaunchKernelGGL(k_scatter_perm, dim3(gb), dim3(256), 0, s, c->NV, c->perm.p, c->v_x.p, x);
  HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int tsl_solve(tsl_ctx* c, const double* rhs, double* x, tsl_solve_stats* st) {
  Scope scope(c);
  TSL_TRY(solve_orig(c, rhs, x, st));
  HIP_OK(hipStreamSynchronize(c->stream));
  return 0;
}

#include "param_api.hpp"
#include "mg_test_api.hpp"
#include "op_test_api.hpp"

// ------------------------------------------------------------------------------------------------
extern "C" int tsl_update_ref_angle(tsl_ctx* c, const double* pos, double* ref) {
  Scope scope(c);
  if (!c->n_hinge) return 0;
  hipStream_t s = c->stream;
  hipLaunchKernelGGL(k_cloth_normals, dim3(nblk(c->n_cface, 256)), dim3(256), 0, s, c->n_cface, pos, c->cf_f2v.p, c->norm_dir.p);
  hipLaunchKernelGGL(k_cloth_update_ref, dim3(nblk(c->n_hinge, 256)), dim3(256), 0, s, cloth_args(c), pos, ref);
  HIP_OK(hipGetLastError());
  return 0;
}

// One time step (BaseScene.py:1327-1370) of every member of `m` in LOCK STEP.  Every phase of a Newton iteration is issued for all members before
// any of them is waited for -- energies, assemblies, the line-search trials -- and every decision per member (line-search halving, Newton stop rule)
// is that of the member stepped alone.  The linear solve is the one phase that differs: `solve` takes the members of `act` from the right-hand sides
// gathered into their v_b to their directions in pdir (ss[i]: member i's statistics) and may time its parts with lap(2..5).  tsl_step is the loop
// with one member and its own solve, tsl_group_step the loop with the group's members and the merged solve.
struct StepMember { tsl_ctx* c; double *pos, *prev, *vel, *ref; };
using StepSolve = std::function<int(const std::vector<int>& act, std::vector<tsl_solve_stats>& ss, const std::function<void(int)>& lap)>;

static void add_solve_stats(tsl_step_stats& t, const tsl_solve_stats& s) {
  t.cg_iters += s.iters; t.solves++; t.restarts += s.restarts; t.fallback += (s.flag == 1); t.unconverged += (s.flag == 3); t.attained += s.attained;
  t.max_rel_residual = std::max(t.max_rel_residual, s.rel_residual); t.max_backward_error = std::max(t.max_backward_error, s.backward_error);
}

// pool: host threads that issue the members' assemblies side by side (nullptr: one after the other on this thread); g: the pseudo-context of a
// group's merged solver (nullptr for a scene alone): its stream is waited for with the members', its factorisations count with member 0's
static int newton_step(const std::vector<StepMember>& m, GroupPool* pool, tsl_ctx* g, const StepSolve& solve, tsl_step_stats* stats) {
  const int n = (int)m.size();
  struct InStep { const std::vector<StepMember>& m; ~InStep() { for (const StepMember& e : m) { e.c->in_step = false; e.c->st_pos = nullptr; } } } guard{m};
  std::vector<tsl_step_stats> st(n);
  std::vector<long> fact0(n), plans0(n);
  std::vector<int> iter(n, 0), active(n, 1);
  std::vector<double> delta(n, 1e5), E0(n, 0.0), E(n, 0.0), alpha(n, 1.0);
  for (int i = 0; i < n; i++) {
    tsl_ctx* c = m[i].c;
    memset(&st[i], 0, sizeof(tsl_step_stats));
    fact0[i] = c->ds.n_factor; plans0[i] = c->ds.n_plans;
    c->in_step = true; c->mg_omega_valid = false; c->tm_loop = 0;
    // level solved exactly by the multigrid cycle: a dense inverse per assembly pays for a ~840-node level (2.5k unknowns, some ms
    // per inversion) only when the solves are long -- decided from the previous time step (cfg4: 300 -> 220 iterations per solve
    // at +4.5 ms per assembly; the scaled scene with ~100 iterations per solve keeps the 225-node level)
    // -- and a step whose predecessor needed fewer than 60 keeps the hierarchy down to the 64-node level, whose inverse is one
    // single-workgroup kernel (drape: 25 iterations per solve, a 1 ms inversion per assembly would cost 15 % of the step)
    // The thresholds to LEAVE a tier downwards are 40 % lower than the ones to enter it: the larger dense level itself lowers the
    // count (cfg4: 257 iterations per solve on the 225-node tier, 197 on the 841-node tier), and a rule without hysteresis flips
    // between the tiers from step to step (measured: 55.8k element-steps/s flipping, 62.7k staying on the 841-node level).
    if (c->mg_dense_auto) {
      const double it = c->last_step_iters_per_solve;
      const int cur = c->mg_dense_nodes;
      const double to_900 = cur >= 900 ? 120.0 : 200.0, to_256 = cur >= 256 ? 36.0 : 60.0;
      c->mg_dense_nodes = it > to_900 ? 900 : it > to_256 ? 256 : 64;
    }
    if (c->ds.hard && ++c->ds.hard_steps > c->ds.probe_every) c->ds.hard = false;   // probe the iterative hierarchy again
    c->bd_valid = false;  // dense body inverses are rebuilt once per step (first solve) and lagged over its Newton iterations
    // timestep_init: prev_pos <- pos (BaseScene.py:1291-1303)
    HIP_OK(hipMemcpyAsync(m[i].prev, m[i].pos, 3 * (size_t)c->NV * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  }
  for (int i = 0; i < n; i++) {   // calc_vn + projection_query + contact_analysis
    tsl_ctx* c = m[i].c;
    int nc = 0;
    if (c->contact_enable) TSL_TRY(tsl_contact_detect(c, m[i].pos, m[i].prev, &nc));
    else TSL_TRY(contact_slots_none(c));
    st[i].nc = nc;
  }
  const long gfact0 = g ? g->ds.n_factor : 0;
  // verbose: host wall time per phase (every phase ends in a synchronisation of all streams when timed): energy, assembly + preconditioner set-up,
  // the merged solve's plans + merge, factorisation and application, the rest of the solves, line search
  const bool timed = m[0].c->verbose >= 1;
  double tph[7] = {0, 0, 0, 0, 0, 0, 0};
  auto tick = std::chrono::steady_clock::now();
  const std::function<void(int)> lap = [&](int k) { if (!timed) return; for (const StepMember& e : m) (void)hipStreamSynchronize(e.c->stream); if (g) (void)hipStreamSynchronize(g->stream);
                                                     const auto nw = std::chrono::steady_clock::now(); if (k >= 0) tph[k] += std::chrono::duration<double>(nw - tick).count(); tick = nw; };
  auto energy_issue = [&](int i) -> int {   // energy of member i's positions -> its host scalars (read after a synchronisation of its stream)
    tsl_ctx* c = m[i].c;
    TSL_TRY(energy_async(c, m[i].pos, m[i].prev, m[i].vel, m[i].ref));
    HIP_OK(hipMemcpyAsync(&HSC(c)->energy, &SC(c)->energy, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return 0;
  };
  const std::function<int(int)> assemble_one = [&](int i) -> int {
    tsl_ctx* c = m[i].c;
    TSL_TRY(assemble(c, m[i].pos, m[i].prev, m[i].vel, m[i].ref, 1, c->F.p));
    hipLaunchKernelGGL(k_gather_perm, dim3(nblk(c->NV, 256)), dim3(256), 0, c->stream, c->NV, c->perm.p, (const double*)c->F.p, c->v_b.p);
    return 0;
  };
  std::vector<tsl_solve_stats> ss(n);
  lap(-1);
  for (;;) {
    std::vector<int> act;
    for (int i = 0; i < n; i++) if (active[i] && iter[i] < m[i].c->newton_cap) act.push_back(i);
    if (act.empty()) break;
    // compute_energy at the top of an iteration (BaseScene time_step): the state is the one the previous line search ended on, whose
    // energy is known (same kernel, same positions) -- evaluated anew only in the first iteration
    for (int i : act) if (++iter[i] == 1) TSL_TRY(energy_issue(i));
    for (int i : act) { if (iter[i] == 1) { HIP_OK(hipStreamSynchronize(m[i].c->stream)); E0[i] = HSC(m[i].c)->energy; } else E0[i] = E[i]; }
    lap(0);
    if (pool) TSL_TRY(pool->run(act, assemble_one));   // (one host thread per member: the ~35 launches of an assembly are issued side by side)
    else for (int i : act) TSL_TRY(assemble_one(i));
    lap(1);
    TSL_TRY(solve(act, ss, lap));
    lap(5);
    for (int i : act) {
      tsl_ctx* c = m[i].c;
      const size_t n3 = 3 * (size_t)c->NV;
      hipStream_t s = c->stream;
      add_solve_stats(st[i], ss[i]);
      // p_norm = max |p|  (calc_p_norm :1096-1103): the refinement of the factorised solve delivers it with its last residual; other solvers: one reduction
      const bool have_pmax = ss[i].method == 4 && ss[i].flag == 0 && c->last_xmax_valid;
      if (have_pmax) HSC(c)->pmax = c->last_xmax;
      else {
        HIP_OK(hipMemsetAsync(&SC(c)->pmax, 0, sizeof(double), s));
        hipLaunchKernelGGL(k_absmax, dim3(gsz(n3)), dim3(256), 0, s, n3, c->pdir.p, &SC(c)->pmax);
        HIP_OK(hipMemcpyAsync(&HSC(c)->pmax, &SC(c)->pmax, sizeof(double), hipMemcpyDeviceToHost, s));
      }
      HIP_OK(hipMemcpyAsync(c->x1.p, m[i].pos, n3 * sizeof(double), hipMemcpyDeviceToDevice, s));
      alpha[i] = 1.0;
    }
    // halving line search: every pending member's trial is issued before any of them is read
    std::vector<int> pend = act;
    while (!pend.empty()) {
      for (int i : pend) {
        tsl_ctx* c = m[i].c;
        const size_t n3 = 3 * (size_t)c->NV;
        hipLaunchKernelGGL(k_linesearch, dim3(gsz(n3)), dim3(256), 0, c->stream, n3, c->x1.p, c->pdir.p, alpha[i], m[i].pos);
        TSL_TRY(energy_issue(i));
      }
      std::vector<int> again;
      for (int i : pend) {
        HIP_OK(hipStreamSynchronize(m[i].c->stream));
        E[i] = HSC(m[i].c)->energy;
        st[i].ls_evals++;
        if (E[i] < E0[i]) continue;
        alpha[i] /= 2;
        if (alpha[i] > 1e-8) again.push_back(i);
      }
      pend.swap(again);
    }
    for (int i : act) {
      tsl_ctx* c = m[i].c;
      delta[i] = HSC(c)->pmax / c->dt;   // copied before the line search; its energy evaluations synchronised the stream since
      st[i].last_alpha = alpha[i]; st[i].energy = E[i];
      if (c->verbose >= 4) fprintf(stderr, "[tsl]   scene %d newton %2d: E0 %.12e  E - E0 %+.3e  alpha %.3g  |p|max %.3e  delta %.3e  (solve: %d its, rel_residual %.1e)\n", i, iter[i], E0[i], E[i] - E0[i], alpha[i],
                                   HSC(c)->pmax, delta[i], ss[i].iters, ss[i].rel_residual);
      if (delta[i] < 1e-7) active[i] = 0;
    }
    lap(6);
  }
  if (timed) {
    long its = 0;
    double loops = 0;
    for (int i = 0; i < n; i++) { its += st[i].cg_iters; loops += m[i].c->tm_loop; }
    fprintf(stderr, "[tsl] step of %d scene(s): %d Newton iterations (most of a scene), %ld solver iterations; energy %.3f s, assembly + preconditioner set-up %.3f s, solves %.3f s "
            "(merged plans + merge %.3f s, factorisation %.3f s, application %.3f s; iteration loops %.3f s), line search %.3f s\n",
            n, *std::max_element(iter.begin(), iter.end()), its, tph[0], tph[1], tph[2] + tph[3] + tph[4] + tph[5], tph[2], tph[3], tph[4], loops, tph[6]);
  }
  for (int i = 0; i < n; i++) {
    tsl_ctx* c = m[i].c;
    const size_t n3 = 3 * (size_t)c->NV;
    st[i].newton_iters = iter[i]; st[i].last_delta = delta[i];
    st[i].factorizations = (int)(c->ds.n_factor - fact0[i]) + (g && i == 0 ? (int)(g->ds.n_factor - gfact0) : 0); st[i].plans = (int)(c->ds.n_plans - plans0[i]);
    // timestep_finish: update_vel (+ plastic update_ref_angle, Scene_folding.py:227-231)
    hipLaunchKernelGGL(k_update_vel, dim3(gsz(n3)), dim3(256), 0, c->stream, n3, m[i].pos, m[i].prev, c->damping / c->dt, m[i].vel);
    if (c->plastic) TSL_TRY(tsl_update_ref_angle(c, m[i].pos, m[i].ref));
  }
  for (int i = 0; i < n; i++) {
    tsl_ctx* c = m[i].c;
    HIP_OK(hipStreamSynchronize(c->stream));
    if (st[i].solves > 0) c->last_step_iters_per_solve = (double)st[i].cg_iters / st[i].solves;
    if (stats) stats[i] = st[i];
  }
  if (g) HIP_OK(hipStreamSynchronize(g->stream));
  HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int tsl_step(tsl_ctx* c, double* pos, double* prev, double* vel, double* ref, tsl_step_stats* stats) {
  Scope scope(c);
  const StepSolve solve = [c](const std::vector<int>&, std::vector<tsl_solve_stats>& ss, const std::function<void(int)>&) -> int {
    TSL_TRY(solve_perm(c, &ss[0]));
    hipLaunchKernelGGL(k_scatter_perm, dim3(nblk(c->NV, 256)), dim3(256), 0, c->stream, c->NV, c->perm.p, (const double*)c->v_x.p, c->pdir.p);
    HIP_OK(hipGetLastError());
    if (ss[0].method == 4) TSL_TRY(direct_prezero(c));   // the factors are not needed again: clear the arena for the next iteration next to the line search
    return 0;
  };
  return newton_step({StepMember{c, pos, prev, vel, ref}}, nullptr, nullptr, solve, stats);
}

// ------------------------------------------------------------------------------------------------
// Scene group (direct_group.hpp): S scenes of one GPU stepped in LOCK STEP by one host thread through tsl_step's Newton loop (newton_step); the
// sparse direct solves of all members are ONE factorisation and ONE application of the merged plan on the group's stream.  Per member the sequence
// of kernels, their arguments and every decision (first-pass verdict, line-search halving, Newton stop rule) are those of tsl_step, so a member's
// tape is bit-identical to its single-scene run.  A member whose merged first pass is not accepted goes on from it through its own solve path
// (its plan addresses the same factors).
static std::mutex g_group_mu;
static std::vector<tsl_group*> g_groups;
static void group_unregister_and_destroy(tsl_group* G) {
  { std::lock_guard<std::mutex> lk(g_group_mu);
    auto it = std::find(g_groups.begin(), g_groups.end(), G);
    if (it == g_groups.end()) return;
    g_groups.erase(it); }
  group_destroy(G);
}
extern "C" int tsl_group_create(tsl_ctx* const* ctxs, int32_t n, tsl_group** out) {
  for (int i = 0; i < n; i++) if (!direct_enabled(ctxs[i])) return tsl_fail("tsl_group_create: scene %d does not use the sparse direct solve (\"direct\" = 1 or a cloth grid of >= 1024 cells)", i);
  TSL_TRY(group_create(ctxs, n, out));
  std::lock_guard<std::mutex> lk(g_group_mu);
  g_groups.push_back(*out);
  return 0;
}
extern "C" void tsl_group_destroy(tsl_group* G) { if (G) group_unregister_and_destroy(G); }
// {merges of the members' plans, re-layouts of the group's arenas, host seconds in merges, bytes of the group's arenas, factorisations and applications of the merged plan,
// solves in which a member went on from the merged first pass on its own path, dataflow launches of the merged factorisations, merged factorisations redone on the
// block-step path after such a launch lost a flag}
extern "C" int tsl_group_info(tsl_group* G, double* out9) {   // (nine values)
  out9[0] = (double)G->n_merge; out9[1] = (double)G->n_relayout; out9[2] = G->t_merge; out9[3] = 8.0 * (double)(G->arena.n + G->sarena.n + G->garena.n + G->w.n);
  out9[4] = (double)G->g->ds.n_factor; out9[5] = (double)G->g->ds.n_apply; out9[6] = (double)G->n_own_path;
  out9[7] = (double)G->g->ds.n_flow; out9[8] = (double)G->g->ds.n_flow_abort;
  return 0;
}

// The merged solve of a scene group: v_x <- H^-1 v_b for the members in `act` (permuted order; every member has assembled its operator and gathered
// its right-hand side on its own stream).  Plans (and the merge when one changed), ONE factorisation and ONE first application for all members,
// then per member the residual and the verdict on that first pass (ir_pass_enqueue / ir_pass_verdict, as in direct_refine) and -- where it does not
// settle -- the member's own solve path from the second pass on.  ss[i] = the solve statistics of member i; lap(2..5) times the parts.
static int group_solve(tsl_group* G, const std::vector<int>& act, std::vector<tsl_solve_stats>& ss, const std::function<void(int)>& lap) {
  const int n = (int)G->m.size();
  tsl_ctx* g = G->g;
  // ---- plans: every member's own (rebuilt when its constraint set changed: once per time step), then the merge
  {
    std::vector<int> todo;   // (members whose constraint set has not been looked at since the last detection: the first solve of a time step / adjoint step)
    for (int i = 0; i < n; i++) { tsl_ctx* c = G->m[i]; if (!(c->ds.plan_valid && c->ds.cons_checked)) todo.push_back(i); }
    if (todo.size() > 1) TSL_TRY(G->pool->run(todo, [&](int i) -> int { return direct_plan(G->m[i]); }));   // side by side: a plan is ~5 ms of host work
    for (int i = 0; i < n; i++) TSL_TRY(direct_plan(G->m[i]));
  }
  bool stale = !G->merged_valid;
  for (int i = 0; i < n; i++) stale |= G->seen_gen[i] != G->m[i]->ds.plan_gen;
  if (stale) {
    for (int i = 0; i < n; i++) HIP_OK(hipStreamSynchronize(G->m[i]->stream));
    TSL_TRY(group_merge(G));
  }
  lap(2);
  // ---- the merged solver takes its tuning from the members at every solve (a tsl_set_param on a member after the group was formed must not be lost: a stale
  // piv_tol changes the factors, and with them the promise that a member's tape equals its single-scene run); members that disagree are an error
  {
    DirectSolver& gd = g->ds;
    const DirectSolver& d0 = G->m[0]->ds;
    for (int i = 1; i < n; i++) {
      const DirectSolver& di = G->m[i]->ds;
      if (di.piv_tol != d0.piv_tol || di.flow != d0.flow || di.g32_below != d0.g32_below || di.gemv_wide_below != d0.gemv_wide_below || di.small_rounds != d0.small_rounds)
        return tsl_fail("scene group: members 0 and %d differ in a parameter of the factorisation (direct_piv_tol / _flow / _g32_below / _gemv_wide_below / _small_rounds)", i);
    }
    if (gd.piv_tol != d0.piv_tol) gd.piv_tol = d0.piv_tol;
    gd.flow = G->flow_lost ? 0 : d0.flow; gd.g32_below = d0.g32_below; gd.gemv_wide_below = d0.gemv_wide_below; gd.small_rounds = d0.small_rounds * n; gd.xcd_map = d0.xcd_map;
    gd.prezero = d0.prezero; gd.dbg = d0.dbg;
  }
  // ---- ONE factorisation and ONE application for all members, the verdict on the first pass per member.  A dataflow launch of the MERGED factorisation that
  // lost a flag leaves garbage factors for every member (solve_perm's abort check looks at the member's own counters, which the merged launch never touched):
  // before any member is sent down its own path the merged launch's abort word is read, and on an abort the merged factorisation runs once more on the
  // launch-per-block-step path
  ss.assign(n, tsl_solve_stats{});
  std::vector<char> okv(n, 1);
  for (int attempt = 0; attempt < 2; attempt++) {
    DirectSolver& gd = g->ds;
    for (int i = 0; i < n; i++) { HIP_OK(hipEventRecord(G->ev_m[i], G->m[i]->stream)); HIP_OK(hipStreamWaitEvent(g->stream, G->ev_m[i], 0)); }
    gd.numeric_valid = false;
    if (attempt > 0) {
      gd.have_factor = false;   // the factors in place are garbage: direct_factor must not return early
      if (gd.prezero_pending) { HIP_OK(hipStreamWaitEvent(g->stream, gd.ev_zero, 0)); gd.prezero_pending = false; }
    }
    TSL_TRY(direct_factor(g));
    if (attempt == 0) for (int i = 0; i < n; i++) { DirectSolver& d = G->m[i]->ds; if (++d.anorm_age >= 64) d.anorm_valid = false; }   // (the members never call direct_factor: |H|_inf ages here)
    lap(3);
    TSL_TRY(direct_apply(g, G->vb.p, G->vx.p));
    HIP_OK(hipEventRecord(G->ev_g, g->stream));
    lap(4);
    for (int i = 0; i < n; i++) HIP_OK(hipStreamWaitEvent(G->m[i]->stream, G->ev_g, 0));
    for (int i : act) TSL_TRY(ir_pass_enqueue(G->m[i]));
    bool any_bad = false;
    for (int i : act) {
      tsl_ctx* c = G->m[i];
      HIP_OK(hipStreamSynchronize(c->stream));
      ss[i] = tsl_solve_stats{};
      const int ok = ir_pass_verdict(c, &ss[i], true);
      if (ok < 0) return -1;
      okv[i] = (char)ok;
      any_bad |= !ok;
    }
    if (attempt == 0) {
      int note[8];
      const int lost = ds_flow_lost(g, any_bad, note);
      if (lost < 0) return -1;
      if (lost) {
        fprintf(stderr, "[tsl] scene group: k_ds_gj_flow of the merged factorisation waited in vain for a flag: \"direct_flow\" disabled for the group, refactorising "
                "(workgroup %d of %d gave up; flag value %d, epoch %d)\n", note[2], note[1], note[3], note[4]);
        gd.flow = 0; gd.n_flow_abort++; G->flow_lost = true;
        continue;
      }
    }
    break;
  }
  for (int i : act) {
    tsl_ctx* c = G->m[i];
    tsl_solve_stats& s1 = ss[i];
    if (okv[i]) { s1.flag = 0; s1.method = 4; continue; }
    // The merged factorisation IS the member's factorisation (its own plan addresses the same memory in the same layout): the member goes on
    // from the merged first pass on its own path -- refinement from the second pass, flexible GMRES and the hierarchy behind it (solve_perm) if
    // that does not settle.  (The group's clear of the leaf panels is issued after these, below.)
    c->ds.numeric_valid = true; c->ds.have_factor = true;
    const tsl_solve_stats first = s1;
    TSL_TRY(solve_perm(c, &s1, &first));
    G->n_own_path++;
    if (c->verbose >= 2) fprintf(stderr, "[tsl] scene group: member %d went on from the merged pass (rel_residual %.2e) on its own path: flag %d after %d applications\n", i, first.rel_residual, s1.flag, s1.iters);
  }
  for (int i = 0; i < n; i++) { tsl_ctx* c = G->m[i]; c->ds.numeric_valid = false; c->ds.have_factor = false; HIP_OK(hipEventRecord(G->ev_m[i], c->stream)); HIP_OK(hipStreamWaitEvent(g->stream, G->ev_m[i], 0)); }
  TSL_TRY(direct_prezero(g));   // the factors are dead: the leaf panels of the next factorisation are cleared next to the line search and the next assembly
  lap(5);
  return 0;
}

extern "C" int tsl_group_step(tsl_group* G, double* const* pos_a, double* const* prev_a, double* const* vel_a, double* const* ref_a, tsl_step_stats* stats) {
  const int n = (int)G->m.size();
  std::vector<std::unique_ptr<Scope>> scopes;
  for (int i = 0; i < n; i++) scopes.emplace_back(new Scope(G->m[i]));
  std::vector<StepMember> m(n);
  for (int i = 0; i < n; i++) {
    if (!direct_enabled(G->m[i])) return tsl_fail("tsl_group_step: scene %d does not use the sparse direct solve", i);
    m[i] = StepMember{G->m[i], pos_a[i], prev_a[i], vel_a[i], ref_a[i]};
  }
  G->g->verbose = G->m[0]->verbose;
  const StepSolve solve = [G](const std::vector<int>& act, std::vector<tsl_solve_stats>& ss, const std::function<void(int)>& lap) -> int {
    TSL_TRY(group_solve(G, act, ss, lap));
    for (int i : act) {
      tsl_ctx* c = G->m[i];
      hipLaunchKernelGGL(k_scatter_perm, dim3(nblk(c->NV, 256)), dim3(256), 0, c->stream, c->NV, c->perm.p, (const double*)c->v_x.p, c->pdir.p);
    }
    return 0;
  };
  return newton_step(m, G->pool.get(), G->g, solve, stats);
}

// ------------------------------------------------------------------------------------------------
extern "C" int tsl_matrix_nnzb(tsl_ctx* c, int32_t* nb, int32_t* nnzb) {
  *nb = c->NV; *nnzb = (int32_t)c->nnzb;
  return 0;
}

// masked system matrix (what tsl_solve inverts) + the matrix-free contact blocks, as BSR in the original ordering
extern "C" int tsl_matrix_export(tsl_ctx* c, int32_t* row_ptr, int32_t* col, double* vals) {
  Scope scope(c);
  HIP_OK(hipStreamSynchronize(c->stream));
  std::vector<double> hv(c->vals.n);
  HIP_OK(hipMemcpy(hv.data(), c->vals.p, hv.size() * sizeof(double), hipMemcpyDeviceToHost));
  long k = 0;
  row_ptr[0] = 0;
  for (int v = 0; v < c->NV; v++) {
    const auto& r = c->h_rows[v];
    const int p = c->h_rowpos[v], s = p >> 6, lane = p & 63;
    for (size_t j = 0; j < r.size(); j++, k++) {
      col[k] = r[j];
      const size_t base = ((size_t)c->h_slice_off[s] + 64 * j) * 9 + lane;
      for (int e = 0; e < 9; e++) vals[9 * k + e] = hv[base + 64 * e];
    }
    row_ptr[v + 1] = (int32_t)k;
  }
  return 0;
}

// the inverse of tsl_matrix_export: BSR values in exactly the pattern and order it returns, written into the SELL layout of the static
// part; the contact blocks of the last detection stay as they are.  Everything built from the values is marked stale, as an assembly does.
extern "C" int tsl_matrix_import(tsl_ctx* c, const double* vals) {
  Scope scope(c);
  HIP_OK(hipStreamSynchronize(c->stream));
  std::vector<double> hv(c->vals.n);
  HIP_OK(hipMemcpy(hv.data(), c->vals.p, hv.size() * sizeof(double), hipMemcpyDeviceToHost));
  long k = 0;
  for (int v = 0; v < c->NV; v++) {
    const int p = c->h_rowpos[v], s = p >> 6, lane = p & 63;
    for (size_t j = 0; j < c->h_rows[v].size(); j++, k++) {
      const size_t base = ((size_t)c->h_slice_off[s] + 64 * j) * 9 + lane;
      for (int e = 0; e < 9; e++) hv[base + 64 * e] = vals[9 * k + e];
    }
  }
  HIP_OK(hipMemcpy(c->vals.p, hv.data(), hv.size() * sizeof(double), hipMemcpyHostToDevice));
  c->ds.numeric_valid = false; c->ds.anorm_valid = false;
  c->mg_ops_valid = false; c->pc_separate = false;
  c->bd_valid = false; c->mg_omega_valid = false;
  c->dinv_valid = false;   // the block-Jacobi inverse too: block_jacobi_ensure kept the one of the values before (c_diag holds contact blocks only: it stays)
  return 0;
}

extern "C" int tsl_profile_reset(tsl_ctx* c, int enable) {
  c->prof_enable = enable; c->prof_ms = 0; c->prof_chunks = 0; c->ev_sample_next = false; c->prof_launches = 0; c->prof_samples = 0; c->ev_used = 0; c->prof_dev_used = 0; c->prof_dev_ticks = 0; c->prof_dev_n = 0;
  if (enable) {
    c->prof_waves = (size_t)c->n_slices * PCG_WPS;
    c->prof_dev_cap = 1;
    if (c->prof_dev.n == 0) TSL_TRY(c->prof_dev.alloc(2 * c->prof_waves * (size_t)c->prof_dev_cap));
    HIP_OK(hipMemset(c->prof_dev.p, 0, c->prof_dev.n * sizeof(unsigned long long)));
  }
  if (enable && c->ev_pool.empty()) {
    for (int i = 0; i < 64; i++) {
      hipEvent_t a, b;
      HIP_OK(hipEventCreate(&a)); HIP_OK(hipEventCreate(&b));
      c->ev_pool.push_back({a, b});
    }
  }
  return 0;
}

extern "C" int tsl_profile_read(tsl_ctx* c, double* ms_per_launch, int64_t* launches, int64_t* bytes_per_launch) {
  Scope scope(c);
  HIP_OK(hipStreamSynchronize(c->stream));
  prof_collect(c);
  // device-clock spans of the sampled launches (what a kernel trace reports as the kernel duration)
  double dev_ms = 0;
  long n_dev = c->prof_dev_n;
  {
    int dev = 0, khz = 100000;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0) khz = 100000;
    dev_ms = c->prof_dev_ticks / (double)khz;
  }
  c->prof_event_ms = c->prof_samples ? c->prof_ms / c->prof_samples : 0.0;
  *ms_per_launch = n_dev ? dev_ms / n_dev : c->prof_event_ms;
  *launches = c->prof_launches;
  // algorithmic bytes of one SpMV: every stored block (72 B values + 4 B column id) + x gather + y store per row
  *bytes_per_launch = (int64_t)c->nnzb * 76 + (int64_t)c->NV * (24 + 24);
  return 0;
}

extern "C" int tsl_profile_read_events(tsl_ctx* c, double* ms_per_launch_events) {
  *ms_per_launch_events = c->prof_event_ms;
  return 0;
}

// micro-benchmark of the SpMV variants on the currently assembled matrix: average microseconds per launch over reps
// back-to-back launches bracketed by one hipEvent pair (includes ~1.5 us dependent-launch gaps)
extern "C" int tsl_bench_spmv(tsl_ctx* c, int variant, int reps, double* us_per_launch) {
  Scope scope(c);
  hipStream_t s = c->stream;
  hipEvent_t e0, e1;
  HIP_OK(hipEventCreate(&e0)); HIP_OK(hipEventCreate(&e1));
  const int ns = c->n_slices;
  if (c->v_t4.n < (size_t)ns) return tsl_fail("scratch too small");
  int k1_count = 0;
  const int variant30_grid = std::min<long>(std::max<long>((long)c->v_t4.n, 1), 2048);
  auto launch = [&]() {
    switch (variant) {
      case 0: case 1: case 2: case 3: case 4: case 5: case 6: case 7: spmv_variant_launch(c, variant, c->v_p.p, c->v_Ap.p, c->v_t4.p); break;
      case 10: hipLaunchKernelGGL(k_spmv, dim3(nblk((long)ns * 64, 256)), dim3(256), 0, s, c->NV, ns, c->slice_off.p, c->slice_len.p, c->colidx.p, c->vals.p, c->v_p.p, c->v_Ap.p, SC(c), 0, 1, (unsigned long long*)nullptr); break;
      case 11: hipLaunchKernelGGL(k_spmv, dim3(nblk((long)ns * 64, 256)), dim3(256), 0, s, c->NV, ns, c->slice_off.p, c->slice_len.p, c->colidx.p, c->vals.p, c->v_p.p, c->v_Ap.p, SC(c), -1, 0, (unsigned long long*)nullptr); break;
      case 12: {  // one full PCG iteration body (never converges: thresh2 = 0)
        hipLaunchKernelGGL(k_spmv, dim3(nblk((long)ns * 64, 256)), dim3(256), 0, s, c->NV, ns, c->slice_off.p, c->slice_len.p, c->colidx.p, c->vals.p, c->v_p.p, c->v_Ap.p, SC(c), 0, 1, (unsigned long long*)nullptr);
        hipLaunchKernelGGL(k_cg_update, dim3(nblk(c->NV, 256)), dim3(256), 0, s, c->NV, c->v_p.p, c->v_Ap.p, c->Dinv.p, c->v_x.p, c->v_r.p, c->v_z.p, SC(c), 0);
        hipLaunchKernelGGL(k_cg_p, dim3(nblk(c->NV, 256)), dim3(256), 0, s, c->NV, c->v_z.p, c->v_p.p, SC(c), 0, 0);
      } break;
      case 13: hipLaunchKernelGGL(k_cg_update, dim3(nblk(c->NV, 256)), dim3(256), 0, s, c->NV, c->v_p.p, c->v_Ap.p, c->Dinv.p, c->v_x.p, c->v_r.p, c->v_z.p, SC(c), 0); break;
      case 14: hipLaunchKernelGGL(k_cg_p, dim3(nblk(c->NV, 256)), dim3(256), 0, s, c->NV, c->v_z.p, c->v_p.p, SC(c), 0, 0); break;
      case 30: {  // streaming read of the matrix values + column ids (the bytes K1 streams), no index chain / gather / reduction
        const size_t nw = c->vals.n / 2;
        const int grid = variant30_grid;
        hipLaunchKernelGGL(k_stream_read, dim3(grid), dim3(256), 0, s, (const double2*)c->vals.p, nw, c->v_t4.p);
      } break;
      case 20: {  // the PCG operator kernel exactly as an iteration launches it (recurrence form, contact rows of the current step)
        const int par = (k1_count++) & 1;
        hipLaunchKernelGGL((k_pcg_spmv<PCG_WPS, TSL_NT>), dim3(ns), dim3(64 * PCG_WPS), 0, s, c->NV, ns, c->slice_off.p, c->slice_len.p, c->colidx.p, c->vals.p, c->v_z.p,
                           par ? c->v_p.p : c->v_t0.p, par ? c->v_t0.p : c->v_p.p, c->v_Ap.p, c->part_rz.p, c->part_rr.p, c->part_pAp.p, PSC(c), par, 0,
                           (unsigned long long*)nullptr, contact_rows(c, c->c_H.p));
      } break;
      default: break;
    }
  };
  if (variant == 20) {  // state of a running PCG (never converges: thresh2 < 0; beta = 1/2 keeps the direction bounded)
    const size_t n3 = 3 * (size_t)c->NV;
    const int gb = nblk(c->NV, 256);
    std::vector<double> one((size_t)gb, 0.0);
    one[0] = 1.0;
    HIP_OK(hipMemcpyAsync(c->part_rz.p, one.data(), one.size() * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(c->part_rr.p, one.data(), one.size() * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(c->v_z.p, c->v_b.p, n3 * sizeof(double), hipMemcpyDeviceToDevice, s));
    HIP_OK(hipMemsetAsync(c->v_p.p, 0, n3 * sizeof(double), s));
    HIP_OK(hipMemsetAsync(c->v_t0.p, 0, n3 * sizeof(double), s));
    HIP_OK(hipMemsetAsync(c->v_Ap.p, 0, n3 * sizeof(double), s));
    PcgScal hs;
    memset(&hs, 0, sizeof(hs));
    hs.rzh[0] = hs.rzh[1] = 2.0; hs.thresh2 = -1.0; hs.bb = 1.0; hs.n_part1 = ns; hs.n_part2 = gb;
    HIP_OK(hipMemcpyAsync(c->scal.p, &hs, sizeof(PcgScal), hipMemcpyHostToDevice, s));
    HIP_OK(hipStreamSynchronize(s));
  } else
  {  // valid solver state: p = z = r = b (whatever v_b holds, must be non-zero), scalars of a running iteration
    const size_t n3 = 3 * (size_t)c->NV;
    HIP_OK(hipMemcpyAsync(c->v_p.p, c->v_b.p, n3 * sizeof(double), hipMemcpyDeviceToDevice, s));
    HIP_OK(hipMemcpyAsync(c->v_r.p, c->v_b.p, n3 * sizeof(double), hipMemcpyDeviceToDevice, s));
    HIP_OK(hipMemcpyAsync(c->v_z.p, c->v_b.p, n3 * sizeof(double), hipMemcpyDeviceToDevice, s));
    CgScal hs;
    memset(&hs, 0, sizeof(hs));
    hs.rzn[3] = 1e-30; hs.rzn[0] = 1e-30; hs.pAp[0] = 1.0; hs.thresh2 = -1.0;
    HIP_OK(hipMemcpyAsync(c->scal.p, &hs, sizeof(CgScal), hipMemcpyHostToDevice, s));
  }
  for (int i = 0; i < 10; i++) launch();
  HIP_OK(hipEventRecord(e0, s));
  for (int i = 0; i < reps; i++) launch();
  HIP_OK(hipEventRecord(e1, s));
  HIP_OK(hipEventSynchronize(e1));
  float ms = 0;
  HIP_OK(hipEventElapsedTime(&ms, e0, e1));
  *us_per_launch = (double)ms * 1e3 / reps;
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  return 0;
}

extern "C" int tsl_bench_direct(tsl_ctx* c, int cls, int reps, double* out4) {
  Scope scope(c);
  return direct_bench(c, cls, std::max(1, reps), out4);
}

// counters of the direct path since context creation: {plans, factorisations, applications, perturbed pivots of the last
// factorisation, host seconds in plan builds, supernodes, levels, batches, flops per factorisation, bytes of fronts}
extern "C" int tsl_direct_info(tsl_ctx* c, double* out10) {
  Scope scope(c);
  HIP_OK(hipStreamSynchronize(c->stream));
  const DirectSolver& d = c->ds;
  int bad[4] = {0, 0, 0, 0};
  if (d.bad.p) HIP_OK(hipMemcpy(bad, d.bad.p, sizeof(bad), hipMemcpyDeviceToHost));
  out10[0] = (double)d.n_plans; out10[1] = (double)d.n_factor; out10[2] = (double)d.n_apply; out10[3] = bad[1] + bad[2] + bad[3]; out10[4] = d.t_plan;
  out10[5] = d.plan_valid ? d.plan.sym.n_sn : 0; out10[6] = d.plan_valid ? d.plan.n_levels : 0; out10[7] = d.plan_valid ? (double)d.plan.batches.size() : 0;
  out10[8] = d.plan_valid ? d.plan.flops : 0; out10[9] = d.plan_valid ? 8.0 * (double)(d.plan.arena + d.plan.sarena) : 0;
  return 0;
}
// further counters of the direct path, the first n of: {dataflow launches (k_ds_gj_flow), dataflow launches that lost a flag and were redone
// on the block-step path, plans found in the plan cache, bytes of the panel arena (cleared per factorisation), bytes of the Schur arena,
// bytes of the G arena, entries of Schur complements stored per factorisation, plans parked in the cache, first passes of refined solves whose
// componentwise backward error was looked at, first passes accepted on it ("direct_berr"), the largest backward error and the largest forward
// residual so accepted, pivot tiles of the LAST factorisation that failed the static-pivot rule of the cofactor path and were inverted by the guarded form}
extern "C" int tsl_direct_counters(tsl_ctx* c, double* out, int32_t n) {
  const DirectSolver& d = c->ds;
  double e = 0;
  if (d.plan_valid) for (const DsFrontDesc& f : d.plan.fr) e += (double)f.b * f.b;
  size_t parked = 0;
  for (const auto& sl : d.cache) parked += sl->used ? 1 : 0;
  int redo = 0;
  if (n > 12 && d.bad.p) { HIP_OK(hipStreamSynchronize(c->stream)); HIP_OK(hipMemcpy(&redo, d.bad.p + DS_REDO, sizeof(int), hipMemcpyDeviceToHost)); }
  const double v[13] = {(double)d.n_flow, (double)d.n_flow_abort, (double)d.n_plan_hits, d.plan_valid ? 8.0 * (double)d.plan.arena : 0.0, d.plan_valid ? 8.0 * (double)d.plan.sarena : 0.0,
                        d.plan_valid ? 8.0 * (double)d.plan.garena : 0.0, e, (double)parked, (double)d.berr_seen, (double)d.berr_accepted, d.berr_max, d.berr_rel_max, (double)redo};
  for (int i = 0; i < std::min<int>(n, 13); i++) out[i] = v[i];
  return 0;
}

extern "C" int tsl_spd_project(tsl_ctx* c, double* blocks, int32_t n, int32_t D) {
  Scope scope(c);
  if (D != 2 && D != 3 && D != 9) return tsl_fail("tsl_spd_project: D must be 2, 3 or 9");
  if (c->spd_literal && D == 3) hipLaunchKernelGGL(k_spd_batch_literal, dim3(nblk(n, 256)), dim3(256), 0, c->stream, blocks, n, D);
  else if (c->spd_literal && D == 9) hipLaunchKernelGGL(k_spd_batch_literal, dim3(nblk((long)n * 16, 256)), dim3(256), 0, c->stream, blocks, n, D);
  else hipLaunchKernelGGL(k_spd_batch, dim3(nblk(n, 64)), dim3(64), 0, c->stream, blocks, n, D);
  HIP_OK(hipStreamSynchronize(c->stream));
  return 0;
}

#include "adjoint_api.hpp"
