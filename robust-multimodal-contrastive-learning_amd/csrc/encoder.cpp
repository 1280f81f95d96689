// Host-side orchestration of one ViLT encoder pass (forward, data-gradient backward, full backward)
// as a fixed sequence of kernel launches on one HIP stream: no allocation, no synchronisation, so
// the whole pass can be captured into a hipGraph by the caller.
//
// Reference being replaced: ViLTransformerSS.infer / infer_k (vilt/modules/vilt_module.py:275-418),
// VisionTransformer.visual_embed dense case (vision_transformer.py:559-677), Block / Attention / Mlp
// (vision_transformer.py:262-375) and their autograd backward.
#include "rmcl_common.h"
#include "kernels.h"
#include "../../include/rmcl.h"
#include <mutex>

namespace {

// RMCL_MODE_STREAM_ATTN: the attention of a pass runs the streaming kernels (attention_stream.hip) when the bit is set and the pass is
// one the unfused path would otherwise take at bf16 speed settings: N > 256.  Everything else ignores the bit.
inline bool stream_attn(const rmcl_dims& d, int mode_bits) {
  return (mode_bits & RMCL_MODE_STREAM_ATTN) && d.dtype == RMCL_BF16 && !d.exact && d.L + 1 + d.P > 256;
}
// What the last forward left in the `probs` slots of a stash (log-sum-exp or probabilities) and in its `u` slots (the MLP pre-activation
// row-major or in tile order, gemm.h EPI_PREACT_TILED), by stash address: host-side memory of the most recent stashes, so that a
// backward called with the other attention setting is refused instead of reading one as the other, and reads `u` in the layout the
// forward wrote - never one re-derived from tuning keys that may have changed in between.
struct StashNote { const void* stash; bool stream; bool tiled; };
StashNote g_stash_notes[64];
int g_stash_next = 0;
std::mutex g_stash_mu;
// the one lookup (g_stash_mu held): the note of this stash, NULL for a stash the table does not or no longer know
StashNote* find_note(const void* stash) {
  for (auto& n : g_stash_notes)
    if (n.stash == stash) return &n;
  return nullptr;
}
void note_stash(const void* stash, bool stream, bool tiled) {
  std::lock_guard<std::mutex> lk(g_stash_mu);
  StashNote* n = find_note(stash);
  if (!n) { n = &g_stash_notes[g_stash_next]; g_stash_next = (g_stash_next + 1) % 64; }
  *n = StashNote{stash, stream, tiled};
}
// false: a stash this table no longer knows
bool stash_note(const void* stash, StashNote* out) {
  std::lock_guard<std::mutex> lk(g_stash_mu);
  const StashNote* n = find_note(stash);
  if (n) *out = *n;
  return n != nullptr;
}

struct Bump {
  char* base;
  size_t off = 0;
  explicit Bump(void* b) : base(reinterpret_cast<char*>(b)) {}
  template <typename T> T* take(size_t n) {
    off = (off + 255) & ~(size_t)255;
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += n * sizeof(T);
    return p;
  }
  void* take_bytes(size_t n) { return take<char>(n); }
};

inline size_t esz(int dt) { return dt == RMCL_F32 ? 4 : 2; }
inline int ldp_of(int N) { return (N + 7) / 8 * 8; }

#define SLAB_FLOATS(d) ((size_t)4 * (size_t)std::max((d).mlp, (d).patch_k) * (size_t)(d).D)

struct LayerStash {
  float *x_in, *x_mid, *mean1, *rstd1, *mean2, *rstd2;
  void *qkv, *probs, *u, *ao;      // DATA+ (ao: the attention output, for the one-kernel attention backward's delta)
  void* u_t;                       // where the TILED form of u starts (carve_stash), NULL: it has no room in this stash
  void *ln1, *ln2, *h;             // FULL (workspace-aliased otherwise)
};

struct Stash {
  LayerStash layer[64];
  float *x_final, *meanF, *rstdF;
  float *text_e, *text_mean, *text_rstd;
};

struct Work {
  float *scores;      // [B,H,N,ldp] f32 (S and dP)
  float *pe;          // [B*P, D] f32
  void *ln, *ao, *h, *qkv, *probs, *u;   // INFER-mode per-layer temporaries
  float *x_a, *x_b, *x_mid, *stat;       // INFER-mode residual ping-pong + stats
  // backward
  float *dx, *dln, *dxn_full, *de;
  void *dxT, *du, *dqkv, *dao, *dS, *dpe;
  void *dxT2, *du2, *dqkv2;   // second copies: weight-gradient GEMMs read them on the side stream
  void *xb_in, *xb_mid;   // LayerNorm fold: bf16 copies of the residual stream (block input / after attention)
  float *part_in, *part_mid;   // and the per-row partial sums [M][16][2] the producer GEMMs emit
  void* dxT3;         // third dx copy (grouped weight gradients: one launch per layer reads both of the layer's dx copies)
  float* ln_rep;      // LayerNorm dgamma/dbeta replica slots (2 * layers + 1), summed into the arena by the grouped kernel
  float* slab;        // split-K partial slabs of the weight-gradient GEMMs
};

// Stash carve.  INFER: nothing is stashed (everything aliases workspace).
size_t carve_stash(const rmcl_dims& d, int mode, void* base, Stash* st) {
  Bump b(base);
  const size_t M = (size_t)d.B * (d.L + 1 + d.P), D = d.D, N = d.L + 1 + d.P;
  const size_t e = esz(d.dtype);
  if (mode == RMCL_MODE_INFER) return 0;
  for (int l = 0; l < d.layers; ++l) {
    LayerStash ls{};
    ls.x_in = b.take<float>(M * D);
    ls.x_mid = b.take<float>(M * D);
    ls.mean1 = b.take<float>(M); ls.rstd1 = b.take<float>(M);
    ls.mean2 = b.take<float>(M); ls.rstd2 = b.take<float>(M);
    ls.qkv = b.take_bytes(M * 3 * D * e);
    const size_t probs_bytes = (size_t)rmcl_attn_scratch_elems(d.B, d.H, (int)N) * e;
    ls.probs = b.take_bytes(probs_bytes);
    const size_t probs_off = b.off - probs_bytes;
    ls.u = b.take_bytes(M * d.mlp * e);
    const size_t u_off = b.off - M * d.mlp * e;
    // The tiled form of u (gemm.h EPI_PREACT_TILED) holds whole 192-row blocks: (ceil(M / 192) * 192 - M) rows more than the slot.  The stash
    // keeps its size: the tiled buffer starts that much IN FRONT of the slot, in the tail of the `probs` slot before it, and ends where the
    // slot ends.  That tail is free in every pass that takes the tiled form: those are bf16 passes whose attention is fused or streamed
    // (encoder_forward_impl checks it), which keep B * H * NKP fp32 row statistics at the head of `probs` and nothing else.
    {
      const size_t pad = ((((size_t)cdiv((long)M, 192) * 192 - M) * d.mlp * e) + 255) & ~(size_t)255;
      const size_t stat = (size_t)rmcl_attn_stat_elems(d.B, d.H, (int)N) * sizeof(float);
      ls.u_t = (ls.u && d.dtype == RMCL_BF16 && u_off >= probs_off + stat + pad) ? (void*)((char*)ls.u - pad) : nullptr;
    }
    ls.ao = b.take_bytes(M * D * e);
    if (mode == RMCL_MODE_FULL) {
      ls.ln1 = b.take_bytes(M * D * e);
      ls.ln2 = b.take_bytes(M * D * e);
      ls.h = b.take_bytes(M * d.mlp * e);
    }
    if (st) st->layer[l] = ls;
  }
  float* xf = b.take<float>(M * D);
  float* mf = b.take<float>(M);
  float* rf = b.take<float>(M);
  float *te = nullptr, *tm = nullptr, *tr = nullptr;
  {
    te = b.take<float>((size_t)d.B * d.L * D);
    tm = b.take<float>((size_t)d.B * d.L);
    tr = b.take<float>((size_t)d.B * d.L);
  }
  if (st) { st->x_final = xf; st->meanF = mf; st->rstdF = rf; st->text_e = te; st->text_mean = tm; st->text_rstd = tr; }
  return b.off;
}

size_t carve_work(const rmcl_dims& d, void* base, Work* w) {
  Bump b(base);
  const size_t M = (size_t)d.B * (d.L + 1 + d.P), D = d.D, N = d.L + 1 + d.P;
  const size_t e = esz(d.dtype);
  const size_t zn = (size_t)rmcl_attn_scratch_elems(d.B, d.H, (int)N);
  Work k{};
  k.scores = b.take<float>(zn);
  k.pe = b.take<float>((size_t)d.B * d.P * D);
  k.ln = b.take_bytes(M * D * e);
  k.ao = b.take_bytes(M * D * e);
  k.h = b.take_bytes(M * d.mlp * e);
  k.qkv = b.take_bytes(M * 3 * D * e);
  k.probs = b.take_bytes(zn * e);
  k.u = b.take_bytes(M * d.mlp * e);
  k.x_a = b.take<float>(M * D);
  k.x_b = b.take<float>(M * D);
  k.x_mid = b.take<float>(M * D);
  k.stat = b.take<float>(4 * M);
  k.dx = b.take<float>(M * D);
  k.dln = b.take<float>(M * D);
  k.dxn_full = b.take<float>(M * D);
  k.de = b.take<float>((size_t)d.B * d.L * D);
  k.dxT = b.take_bytes(M * D * e);
  k.du = b.take_bytes(M * d.mlp * e);
  k.dqkv = b.take_bytes(M * 3 * D * e);
  k.dao = b.take_bytes(M * D * e);
  k.dS = b.take_bytes(zn * e);
  k.dpe = b.take_bytes((size_t)d.B * d.P * D * e);
  k.slab = b.take<float>(SLAB_FLOATS(d));
  k.dxT2 = b.take_bytes(M * D * e);
  k.du2 = b.take_bytes(M * d.mlp * e);
  k.dqkv2 = b.take_bytes(M * 3 * D * e);
  k.dxT3 = b.take_bytes(M * D * e);
  k.xb_in = b.take_bytes(M * D * 2);
  k.xb_mid = b.take_bytes(M * D * 2);
  k.part_in = b.take<float>(M * 2 * 4 * (D / 192 + 1));
  k.part_mid = b.take<float>(M * 2 * 4 * (D / 192 + 1));
  k.ln_rep = b.take<float>((size_t)(2 * d.layers + 1) * RMCL_LN_REP_FLOATS);
  if (w) *w = k;
  return b.off;
}

int check_dims(const rmcl_dims* d) {
  RMCL_REQUIRE(d != nullptr, "dims is NULL");
  RMCL_REQUIRE(d->B > 0 && d->L > 0 && d->P > 0 && d->layers > 0 && d->layers <= 64, "bad dims");
  RMCL_REQUIRE(d->D == d->H * 64, "head dim must be 64");
  RMCL_REQUIRE(d->D % 64 == 0 && d->D <= 1024 && d->mlp % 64 == 0 && d->patch_k % 64 == 0, "D/mlp/patch_k must be multiples of 64 (D <= 1024)");
  RMCL_REQUIRE(d->dtype == RMCL_F32 || d->dtype == RMCL_BF16, "bad dtype");
  RMCL_REQUIRE(d->L + 1 + d->P <= 512, "sequence too long (N <= 512)");
  RMCL_REQUIRE(d->n_types == 0 || d->n_types == 2 || d->n_types == 3, "n_types must be 0, 2 or 3");
  RMCL_REQUIRE(d->img_type >= -1 && d->img_type <= 2, "img_type must be -1, 0, 1 or 2");
  RMCL_REQUIRE((d->img_type != 2 && d->img_type != -1) || d->n_types == 3, "img_type 2 / -1 (NLVR2) needs n_types = 3");
  RMCL_REQUIRE(d->img_type != -1 || d->B % 2 == 0, "img_type -1 (pair pass) needs an even B");
  return 0;
}

struct Ctx {
  const rmcl_dims& d;
  const float* P32;
  const void* Plp;
  rmcl_layout lay;
  hipStream_t s;
  int dt;
  // weight matrix (GEMM operand type) and fp32 vector accessors
  const void* W(int64_t off) const {
    return d.dtype == RMCL_BF16 ? (const void*)((const bf16_t*)Plp + off) : (const void*)(P32 + off);
  }
  const float* V(int64_t off) const { return P32 + off; }
  int64_t L(int l, int64_t rel) const { return lay.layer0 + (int64_t)l * lay.layer_stride + rel; }
};

int gemm(const Ctx& c, const GemmArgs& g, int dt_in, int dt_out, int a_kc, int b_kc) {
  return rmcl_launch_gemm(g, dt_in, dt_out, a_kc, b_kc, c.d.exact, c.s);
}

// split-K factor for weight-gradient GEMMs (reduction over tokens): fill ~2 waves of 256 CUs.
int dw_splitk(int Mout, int Nout, int K) {
  const int tiles = cdiv(Mout, 128) * cdiv(Nout, 128);
  int sk = std::max(1, 512 / tiles);
  sk = std::min(sk, std::max(1, K / 256));
  return std::min(sk, 64);
}

// dW[Nout, Kin] += dY[tokens, Nout]^T @ X[tokens, Kin]   (fp32 atomics into the gradient arena)
int gemm_dw(const Ctx& c, const Work& w, const void* dY, const void* X, float* dW, int Nout, int Kin, int tokens) {
  const size_t slab_floats = SLAB_FLOATS(c.d);
  GemmArgs g = gemm_args(dY, X, dW, Nout, Kin, tokens, Nout, Kin, Kin);
  if (!c.d.exact && c.dt == RMCL_BF16 && w.slab) {
    // bf16 MFMA path: split-K over tokens into fp32 slabs + ordered reduce (no float atomics)
    GemmArgs probe = g;
    const int cfg = rmcl_gemm_fast_get_cfg();                       // tune cfg 1..4 pins the 128x128 kernel (tests A/B the two paths)
    if ((cfg < 1 || cfg > 4) && rmcl_gemm_st_supported(probe, 0, 0) && tokens >= 1024) {
      // 192x192 ping-pong tiles, one (tile, K-slice) work item per CU
      const int tiles = (Nout / 192) * (Kin / 192);
      int sk = std::max(1, 256 / tiles);
      sk = std::min<int>(sk, std::max<size_t>(1, slab_floats / ((size_t)Nout * Kin)));
      g.splitk = sk; g.tag = GEMM_TAG_DW;
      return rmcl_launch_gemm_st_slab(g, w.slab, dW, c.s);
    }
    if (rmcl_gemm_fast_supported(probe, c.dt, RMCL_F32, 0, 0)) {
      const int tiles = (Nout / 128) * (Kin / 128);
      int sk = std::max(1, std::min(8, (256 + tiles - 1) / tiles));
      sk = std::min<int>(sk, std::max<size_t>(1, slab_floats / ((size_t)Nout * Kin)));
      sk = std::min(sk, std::max(1, tokens / 64));
      g.splitk = sk; g.tag = GEMM_TAG_DW;
      return rmcl_launch_gemm_fast_slab(g, w.slab, dW, c.s);
    }
  }
  g.epi = EPI_ATOMIC; g.tag = GEMM_TAG_DW;
  g.splitk = dw_splitk(Nout, Kin, tokens);
  if (g.splitk == 1) g.epi = EPI_ACCUM;
  return gemm(c, g, c.dt, RMCL_F32, 0, 0);
}
// The weight gradient of one linear layer Y = X W^T + b on the per-GEMM path: dW += dY^T X and db += the column sums of dY, both on c's stream
int linear_dw(const Ctx& c, const Work& w, const void* dY, const void* X, float* dW, float* db, int Nout, int Kin, int tokens) {
  RMCL_TRY(gemm_dw(c, w, dY, X, dW, Nout, Kin, tokens));
  return rmcl_colsum(dY, Nout, c.dt, db, tokens, Nout, c.s);
}

// The dropout of one pass: threshold p * 2^32 (0: off), 1 / (1 - p) and the pass seed every site's seed derives from.  A mask is a pure function
// of (site seed, element index) (rmcl_common.h), so the backward builds the same value and regenerates the forward's masks.
struct Dropout {
  uint32_t seed, thresh;
  float inv_keep;
  uint32_t site(int layer, int site_id) const { return rmcl_site_seed(seed, layer, site_id); }
  void set(GemmArgs& g, int epi_bit, int layer, int site_id, int row_mul) const {
    if (thresh) { g.epi |= epi_bit; g.drop_seed = site(layer, site_id); g.drop_thresh = thresh; g.drop_inv_keep = inv_keep; g.drop_row_mul = row_mul; }
  }
  // a forward GEMM site.  row_mul: compact row r of the cls-only tail draws the mask of the dense row r * row_mul (gemm.h drop_row_mul)
  void fwd(GemmArgs& g, int layer, int site_id, int row_mul = 1) const { set(g, EPI_DROPOUT, layer, site_id, row_mul); }
  // fc2-dX: the gradient of the hidden activation takes that activation's forward mask
  void bwd(GemmArgs& g, int layer, int row_mul = 0) const { set(g, EPI_DROP_BWD, layer, DROP_SITE_HIDDEN, row_mul); }
};
int make_dropout(uint32_t seed, float p, bool forward, Dropout* out) {
  if (forward) { RMCL_REQUIRE(p >= 0.f && p < 1.f, "encoder_forward: dropout probability must be in [0,1)"); }
  else { RMCL_REQUIRE(p >= 0.f && p < 1.f, "encoder_backward: dropout probability must be in [0,1)"); }
  *out = Dropout{seed, p > 0.f ? (uint32_t)((double)p * 4294967296.0) : 0u, 1.0f / (1.0f - p)};
  return 0;
}

// ---- the routed GEMM sites of a pass.  ONE builder per site knows its operands, leading dimensions, epilogue bits, ln_* fields and tag, for a
// layer and the pass's switches.  The launch calls it, and so do the routing decisions of the pass (folded, tiled) for layer 0: what a decision
// asked about a GEMM and what the launch then does with it cannot drift apart. ----

// the buffers of one layer in a forward pass: its stash slots, or the workspace where the pass keeps none; x_in is the block's input
struct FwdLayer : LayerStash {
  float* x_out;
  const float* m2_prev;   // LayerNorm 2's row means of the previous layer = the centre the previous fc2 used for this layer's LayerNorm-1 operand
};

struct FwdPass {
  const Ctx& c;
  const Work& w;
  const Stash& st;
  const rmcl_fold* fold;
  int M, D, mlp;
  bool keep, full;              // the pass keeps a stash (DATA, FULL) / also the LayerNorm outputs and h (FULL)
  bool folded, centred, tiled;  // LayerNorm fold, its shift-robust form, tiled pre-activation stash (encoder_forward_impl decides them)
  // A routing decision asks how layer 0's GEMMs WOULD route, on the workspace buffers of a pass without a stash (keep = full = false), in the
  // forms layer 0 may never launch itself: qkv folded (layer 0's own qkv reads the embedding through the LayerNorm kernel), fc1 keeping its
  // pre-activation (C2 = w.u, non-NULL: the 192x192 kernel's rule reads it) and fc2 as a producer even in a one-layer encoder.
  bool probe;
  Dropout drop;
  FwdPass as_probe(bool folded_, bool tiled_) const {
    FwdPass q = *this;
    q.keep = q.full = false; q.probe = true; q.folded = folded_; q.tiled = tiled_;
    return q;
  }

  int fold_rows() const { return 3 * D + mlp; }
  int nparts() const { return 4 * (D / 192); }
  const bf16_t* fold_w(int l, int row) const { return (const bf16_t*)fold->wf + ((long)l * fold_rows() + row) * D; }
  const float* fold_s(int l, int row) const { return fold->sc + (long)l * 2 * fold_rows() + row; }        // s[0..rows), c[rows..2 rows)

  FwdLayer layer(int l, float* x) const {
    void* wu = probe ? w.u : nullptr;
    // (LayerStash in the order of its members: x_in, x_mid, mean1, rstd1, mean2, rstd2, qkv, probs, u, ao, u_t, ln1, ln2, h)
    const LayerStash ws{x, w.x_mid, w.stat, w.stat + M, w.stat + 2 * M, w.stat + 3 * M, w.qkv, w.probs, wu, w.ao, wu, w.ln, w.ln, w.h};
    FwdLayer b{keep ? st.layer[l] : ws, nullptr, nullptr};
    if (!full) { b.ln1 = b.ln2 = w.ln; b.h = w.h; }        // (DATA: the stash has no slots for them)
    b.x_out = keep ? (l + 1 < c.d.layers ? st.layer[l + 1].x_in : st.x_final) : (x == w.x_a ? w.x_b : w.x_a);
    b.m2_prev = l > 0 ? (keep ? st.layer[l - 1].mean2 : w.stat + 2 * M) : nullptr;
    return b;
  }
  // consumer side of the fold: column vectors of W' rows [row, row + N), row statistics from `part`, written to mean / rstd in every mode (the next
  // producer centres on them).  The partials (and the bf16 operand) were taken about `centre`, the row mean of the row's previous LayerNorm.
  void lnfold(GemmArgs& g, int l, int row, float* part, float* mean, float* rstd, const float* centre) const {
    g.ln_s = fold_s(l, row); g.ln_c = fold_s(l, row) + fold_rows(); g.ln_part = part; g.ln_nparts = nparts(); g.ln_cols = D; g.ln_eps = 1e-6f;
    g.ln_mean = mean; g.ln_rstd = rstd; g.ln_center = centred ? centre : nullptr;
  }
  // producer side: the bf16 copy of the output (x - centre) and its per-row partial sums for the next consumer
  void rowstat(GemmArgs& g, void* xb, float* part, const float* centre) const {
    g.epi |= EPI_ROWSTAT; g.C2 = xb; g.ln_part = part; g.ln_nparts = nparts(); g.ln_center = centred ? centre : nullptr;
  }

  GemmArgs qkv(int l, const FwdLayer& b) const {
    if (folded && (l > 0 || probe)) {
      // qkv = LN1(x) Wqkv^T + b: A = the bf16 copy of x the previous fc2 epilogue wrote, row statistics from its partial sums
      GemmArgs g = gemm_args(w.xb_in, fold_w(l, 0), b.qkv, M, 3 * D, D, D, D, 3 * D);
      g.epi = EPI_LNFOLD; g.tag = GEMM_TAG_QKV;
      lnfold(g, l, 0, w.part_in, b.mean1, b.rstd1, b.m2_prev);
      return g;
    }
    GemmArgs g = gemm_args(b.ln1, c.W(c.L(l, c.lay.qkv_w)), b.qkv, M, 3 * D, D, D, D, 3 * D);
    g.epi = EPI_BIAS; g.bias = c.V(c.L(l, c.lay.qkv_b)); g.tag = GEMM_TAG_QKV;
    return g;
  }
  GemmArgs proj(int l, const FwdLayer& b) const {
    GemmArgs g = gemm_args(b.ao, c.W(c.L(l, c.lay.proj_w)), b.x_mid, M, D, D, D, D, D);
    g.epi = EPI_BIAS | EPI_RESIDUAL; g.bias = c.V(c.L(l, c.lay.proj_b)); g.aux = b.x_in; g.ld_aux = D; g.tag = GEMM_TAG_PROJ;
    if (folded) rowstat(g, w.xb_mid, w.part_mid, b.mean1);
    drop.fwd(g, l, DROP_SITE_PROJ);
    return g;
  }
  GemmArgs fc1(int l, const FwdLayer& b) const {
    void* u = tiled ? b.u_t : b.u;                          // (NULL: a pass without a stash keeps no pre-activation)
    GemmArgs g = folded ? gemm_args(w.xb_mid, fold_w(l, 3 * D), b.h, M, mlp, D, D, D, mlp)
                        : gemm_args(b.ln2, c.W(c.L(l, c.lay.fc1_w)), b.h, M, mlp, D, D, D, mlp);
    g.epi = (folded ? EPI_LNFOLD : EPI_BIAS) | EPI_GELU | (u ? EPI_SAVE_PREACT | (tiled ? EPI_PREACT_TILED : 0) : 0); g.C2 = u; g.tag = GEMM_TAG_FC1;
    if (folded) lnfold(g, l, 3 * D, w.part_mid, b.mean2, b.rstd2, b.mean1);
    else g.bias = c.V(c.L(l, c.lay.fc1_b));
    drop.fwd(g, l, DROP_SITE_HIDDEN);
    return g;
  }
  GemmArgs fc2(int l, const FwdLayer& b) const {
    GemmArgs g = gemm_args(b.h, c.W(c.L(l, c.lay.fc2_w)), b.x_out, M, D, mlp, mlp, mlp, D);
    g.epi = EPI_BIAS | EPI_RESIDUAL; g.bias = c.V(c.L(l, c.lay.fc2_b)); g.aux = b.x_mid; g.ld_aux = D; g.tag = GEMM_TAG_FC2;
    if (folded && (l + 1 < c.d.layers || probe)) rowstat(g, w.xb_in, w.part_in, b.mean2);
    drop.fwd(g, l, DROP_SITE_FC2);
    return g;
  }
};

// the four data-gradient GEMMs of a layer, dX = dY W.  The caller names the buffers: the chain rotates them (encoder_backward_impl)
struct BwdSites {
  const Ctx& c;
  int M;
  const void* lpT;     // transposed bf16 weight shadows: dX = dY W as [rows][K] x [cols][K] (W^T stored [in][out], k = out contiguous); NULL: W as it is
  bool u_tiled;        // the `u` slots hold the tiled form (gemm.h EPI_PREACT_TILED)
  Dropout drop;
  int b_kc() const { return lpT ? 1 : 0; }
  GemmArgs dx(const void* dY, int64_t w_off, void* dX, int n_in, int n_out) const {
    const void* W = lpT ? (const void*)((const bf16_t*)lpT + w_off) : c.W(w_off);
    GemmArgs g = gemm_args(dY, W, dX, M, n_in, n_out, n_out, lpT ? n_out : n_in, n_in);
    g.tag = GEMM_TAG_DX;
    return g;
  }
  // du = (dx W2) * gelu'(u) [* hidden mask]
  // (tiled stash: the launch fails with a message when the GEMM no longer routes to the 192x384 kernel - never a row-major read)
  GemmArgs fc2(int l, const void* dY, const void* u, void* du) const {
    GemmArgs g = dx(dY, c.L(l, c.lay.fc2_w), du, c.d.mlp, c.d.D);
    g.epi = EPI_DGELU | (u_tiled ? EPI_PREACT_TILED : 0); g.aux = u; g.ld_aux = c.d.mlp;
    drop.bwd(g, l);
    return g;
  }
  GemmArgs fc1(int l, const void* du, void* dln) const { return dx(du, c.L(l, c.lay.fc1_w), dln, c.d.D, c.d.mlp); }          // dln2 = du W1
  GemmArgs proj(int l, const void* dY, void* dao) const { return dx(dY, c.L(l, c.lay.proj_w), dao, c.d.D, c.d.D); }          // dao = dx Wproj
  GemmArgs qkv(int l, const void* dqkv, void* dln) const { return dx(dqkv, c.L(l, c.lay.qkv_w), dln, c.d.D, 3 * c.d.D); }    // dln1 = dqkv Wqkv
};

// The pixel path's patch rows w.pe: patch GEMM, mask-token substitution, per-sample position rows (encoder forward and rmcl_visual_embed)
int patch_embed(const Ctx& c, const Work& w, const void* patches, const int32_t* replaced, int64_t mask_token_off, const rmcl_ragged* ragged) {
  const rmcl_dims& d = c.d;
  const rmcl_layout& y = c.lay;
  GemmArgs g = gemm_args(patches, c.W(y.patch_w), w.pe, d.B * d.P, d.D, d.patch_k, d.patch_k, d.patch_k, d.D);
  g.epi = EPI_BIAS; g.bias = c.V(y.patch_b); g.tag = GEMM_TAG_PATCH;
  RMCL_TRY(gemm(c, g, c.dt, RMCL_F32, 1, 1));
  // masked patch prediction: the learned mask token takes the place of the replaced patches' embeddings (rmcl_encoder_forward_mpp)
  if (replaced) RMCL_TRY(rmcl_mask_token_fwd(w.pe, replaced, c.V(mask_token_off), d.B * d.P, d.D, c.s));
  if (ragged) {
    // zero-padded batch: per-sample position rows = the table resized to each image's (h, w), gathered at its selected
    // patches (vision_transformer.py:570-600, 645-650); recomputed every pass from the arena of THIS pass (query or momentum)
    RMCL_TRY(rmcl_pos_resize_fwd(c.V(y.pos_img), ragged->sel, ragged->counts, ragged->hw, ragged->sel_ld, ragged->gw, ragged->G0, d.B, d.P, d.D,
                                 ragged->pos_tok, c.s));
  }
  return 0;
}

// cls-only tail of a forward pass (RMCL_MODE_CLS_TAIL), the last block behind its attention: of that block's output only row 0 of every
// sample is read (the pooler takes hidden_states[:, 0], heads.py:17), and everything behind the attention is row-wise - proj, LayerNorm 2,
// the MLP and the final LayerNorm run on the B cls rows (fp32, exact skinny GEMMs) instead of on all B * N tokens.  Compact results live in
// the FIRST B rows of the buffers the dense path would have filled (x_mid, u, h, ln2, x_final, the LN statistics) - the backward with
// cls_only = 2 reads them there.  Dropout: compact row b draws the mask of the dense row b * N it stands for (gemm.h drop_row_mul), so the
// tail gives the dense block's numbers under dropout too.
int forward_tail(const FwdPass& p, int l, const FwdLayer& b, float* xn) {
  const Ctx& c = p.c;
  const Work& w = p.w;
  const rmcl_layout& y = c.lay;
  const int B = c.d.B, N = c.d.L + 1 + c.d.P, D = c.d.D, mlp = c.d.mlp;
  hipStream_t s = c.s;
  float* ao_c = reinterpret_cast<float*>(w.dao);          // backward scratch, free during a forward
  float* ln2_c = reinterpret_cast<float*>(b.ln2);
  float* u_c = reinterpret_cast<float*>(p.keep ? b.u : w.u);              // (always the row-major slot: the compact fp32 u_c is no tiled GEMM stash)
  float* h_c = reinterpret_cast<float*>(b.h);
  float* xo_c = b.x_out;                                   // (a pass with a stash: x_final, this is the last layer)
  {
    // residual operand: the cls rows of the dense residual stream, read in place (row b at b * N * D: no gather launch).  The A
    // operand likewise where the streaming skinny kernel runs the GEMM: the cls rows of the attention output at row stride
    // N * D, bf16 widened in its registers - the bits of the gather-and-cast launch, which only the other forms still need
    GemmArgs g = gemm_args(b.ao, c.V(c.L(l, y.proj_w)), b.x_mid, B, D, D, (long)N * D, D, D);
    g.epi = EPI_BIAS | EPI_RESIDUAL; g.bias = c.V(c.L(l, y.proj_b)); g.aux = b.x_in; g.ld_aux = N * D;
    g.a_bf16 = c.dt == RMCL_BF16;
    p.drop.fwd(g, l, DROP_SITE_PROJ, N);
    if (!rmcl_gemm_skinny_streams(g, 1)) {
      RMCL_TRY(rmcl_rows_gather_cast(b.ao, c.dt, ao_c, B, D, N, 0, s));
      g.A = ao_c; g.lda = D; g.a_bf16 = 0;
    }
    RMCL_TRY(rmcl_launch_gemm_exact(g, RMCL_F32, RMCL_F32, 1, 1, s));
  }
  RMCL_TRY(rmcl_ln_fwd(b.x_mid, D, c.V(c.L(l, y.ln2_w)), c.V(c.L(l, y.ln2_b)), 1e-6f, ln2_c, D, RMCL_F32, b.mean2, b.rstd2, B, D, 0, s));
  {
    GemmArgs g = gemm_args(ln2_c, c.V(c.L(l, y.fc1_w)), h_c, B, mlp, D, D, D, mlp);
    g.epi = EPI_BIAS | EPI_GELU | EPI_SAVE_PREACT; g.bias = c.V(c.L(l, y.fc1_b)); g.C2 = u_c;
    p.drop.fwd(g, l, DROP_SITE_HIDDEN, N);
    RMCL_TRY(rmcl_launch_gemm_exact(g, RMCL_F32, RMCL_F32, 1, 1, s));
  }
  {
    GemmArgs g = gemm_args(h_c, c.V(c.L(l, y.fc2_w)), xo_c, B, D, mlp, mlp, mlp, D);
    g.epi = EPI_BIAS | EPI_RESIDUAL; g.bias = c.V(c.L(l, y.fc2_b)); g.aux = b.x_mid; g.ld_aux = D;
    p.drop.fwd(g, l, DROP_SITE_FC2, N);
    RMCL_TRY(rmcl_launch_gemm_exact(g, RMCL_F32, RMCL_F32, 1, 1, s));
  }
  // final LayerNorm of the cls rows, written to their places in xn (row b * N); the other rows of xn are NOT written
  return rmcl_ln_fwd(xo_c, D, c.V(y.norm_w), c.V(y.norm_b), 1e-6f, xn, (long)N * D, RMCL_F32, p.keep ? p.st.meanF : w.stat,
                     p.keep ? p.st.rstdF : w.stat + p.M, B, D, 0, s);
}

// cls-only tail of a backward pass (cls_only = 2), the last layer behind its attention on the cls rows only: MLP, LayerNorm 2 and proj
// backward on [B, .] fp32 (exact skinny GEMMs); weight / bias gradients of fc2, fc1, proj (G != NULL: FULL mode) reduce over B rows
// instead of B * N; then the two row sets the dense chain continues from are rebuilt: the residual-stream gradient w.dx and d(attention
// output) w.dao, zero except on the cls rows.  dxc: the gradient of the B cls rows [B, D] f32, updated in place.
int backward_tail(const Ctx& c, const Work& w, const LayerStash& ls, int l, float* G, const Dropout& drop, float* dxc) {
  const rmcl_layout& y = c.lay;
  const int B = c.d.B, N = c.d.L + 1 + c.d.P, D = c.d.D, mlp = c.d.mlp, M = B * N;
  hipStream_t s = c.s;
  auto Gp = [&](int64_t rel) { return G + c.L(l, rel); };
  float* u_c = reinterpret_cast<float*>(ls.u);
  float* h_c = reinterpret_cast<float*>(ls.h);
  float* ln2_c = reinterpret_cast<float*>(ls.ln2);
  float* du_c = reinterpret_cast<float*>(w.du);
  float* dln_c = w.dln;
  float* ao_c = reinterpret_cast<float*>(w.dqkv2);
  float* dao_c = reinterpret_cast<float*>(w.du2);
  // dropout: the gradient entering fc2 / proj is the residual-stream gradient times the mask of that branch's output - the mask of
  // the DENSE cls row b * N (forward: drop_row_mul = N); dxc itself keeps flowing down the residual path unmasked
  const float* dy2 = dxc;                                 // d(fc2 output)
  if (drop.thresh) {
    float* m2 = reinterpret_cast<float*>(w.dS);           // (attention-backward scratch: free until the attention backward that follows the tail)
    RMCL_TRY(rmcl_dropout_rows(dxc, m2, B, D, N, drop.site(l, DROP_SITE_FC2), drop.thresh, drop.inv_keep, s));
    dy2 = m2;
  }
  {
    GemmArgs g = gemm_args(dy2, c.V(c.L(l, y.fc2_w)), du_c, B, mlp, D, D, mlp, mlp);                  // du = (dx W2) * gelu'(u) [* hidden mask]
    g.epi = EPI_DGELU; g.aux = u_c; g.ld_aux = mlp;
    drop.bwd(g, l, N);
    RMCL_TRY(rmcl_launch_gemm_exact(g, RMCL_F32, RMCL_F32, 1, 0, s));
  }
  if (G) RMCL_TRY(rmcl_dw_rows(dy2, h_c, Gp(y.fc2_w), Gp(y.fc2_b), D, mlp, B, s));                    // dW2 += dx^T h
  RMCL_TRY(rmcl_launch_gemm_exact(gemm_args(du_c, c.V(c.L(l, y.fc1_w)), dln_c, B, D, mlp, mlp, D, D), RMCL_F32, RMCL_F32, 1, 0, s));   // dln2 = du W1
  if (G) RMCL_TRY(rmcl_dw_rows(du_c, ln2_c, Gp(y.fc1_w), Gp(y.fc1_b), mlp, D, B, s));                 // dW1 += du^T ln2
  RMCL_TRY(rmcl_ln_bwd(dln_c, D, RMCL_F32, ls.x_mid, D, ls.mean2, ls.rstd2, c.V(c.L(l, y.ln2_w)), c.V(c.L(l, y.ln2_b)), dxc, D, 1,
                       G ? Gp(y.ln2_w) : nullptr, G ? Gp(y.ln2_b) : nullptr, B, D, 0, s));   // dxc = d x_mid
  const float* dyp = dxc;                                 // d(proj output)
  if (drop.thresh) {
    float* mp = reinterpret_cast<float*>(w.dS) + (size_t)B * D;
    RMCL_TRY(rmcl_dropout_rows(dxc, mp, B, D, N, drop.site(l, DROP_SITE_PROJ), drop.thresh, drop.inv_keep, s));
    dyp = mp;
  }
  RMCL_TRY(rmcl_launch_gemm_exact(gemm_args(dyp, c.V(c.L(l, y.proj_w)), dao_c, B, D, D, D, D, D), RMCL_F32, RMCL_F32, 1, 0, s));       // dao = dx Wproj
  if (G) {
    RMCL_TRY(rmcl_rows_gather_cast(ls.ao, c.dt, ao_c, B, D, N, 0, s));
    RMCL_TRY(rmcl_dw_rows(dyp, ao_c, Gp(y.proj_w), Gp(y.proj_b), D, D, B, s));                        // dWproj += dx^T ao
  }
  HIP_TRY(hipMemsetAsync(w.dx, 0, (size_t)M * D * sizeof(float), s));
  RMCL_TRY(rmcl_scatter_rows(dxc, w.dx, B, D, 1, N, 0, 0, s));
  HIP_TRY(hipMemsetAsync(w.dao, 0, (size_t)M * D * esz(c.dt), s));
  return rmcl_rows_scatter_cast(dao_c, w.dao, c.dt, B, D, N, 0, s);
}

// ---- side stream for the weight-gradient GEMMs (fills the tile-quantisation tails of the dX chain) ----
hipStream_t g_side = nullptr;
hipEvent_t g_ev[128];
int g_nev = 0;
int ensure_events() {
  for (; g_nev < 128; ++g_nev) HIP_TRY(hipEventCreateWithFlags(&g_ev[g_nev], hipEventDisableTiming));
  return 0;
}
// The events of a weight-gradient backward, one slot per (kind, layer); the ONE place the slot arithmetic lives (encoder_backward_impl
// records and waits, rmcl_grad_ready_wait waits).  EV_FORK is indexed by sub-layer (2 l: MLP, 2 l + 1: attention), the others by layer.
enum EvKind {
  EV_FORK = 0,        // main -> side: the dY of a sub-layer's weight gradients is final
  EV_MLP_DONE = 1,    // side: the MLP weight gradients of a layer are done (its du and dx copy may be rewritten)
  EV_SIDE_DONE = 2,   // side: all weight gradients of a layer are done (attention half on the per-GEMM path; the grouped launch)
  EV_MAIN_DONE = 3,   // main: everything of a layer that runs on the main stream is enqueued
};
hipEvent_t ev_slot(EvKind kind, int idx) { return g_ev[(kind * 32 + (idx & 31)) & 127]; }

}  // namespace

// stash prefetch one layer ahead of the backward chain (rmcl_tune_set key 12: bit 0 = pre-activation u, bit 1 = qkv + attention output,
// bit 2 = the two residual-stream stashes; key 13: workgroups of the touch kernel).  Runs on the stream set by rmcl_set_prefetch_stream.
int g_prefetch_mask = 0, g_prefetch_wgs = 8;
static hipStream_t g_pref = nullptr;
static hipEvent_t g_pev[64];
static int g_npev = 0;
extern "C" int rmcl_set_prefetch_stream(void* stream) { g_pref = (hipStream_t)stream; return 0; }
bool g_lnfold_centred = true;        // rmcl_tune_set key 11: 0 = the uncentred LayerNorm fold of round 2 (A/B, precision tests)
bool rmcl_lnfold_centred() { return g_lnfold_centred; }
bool g_preact_tiled = true;          // rmcl_tune_set key 15: 0 = the MLP pre-activation stash row-major in every pass (A/B, bit-comparison tests)
bool g_dw_grouped = true;            // rmcl_tune_set key 3: 0 selects the per-GEMM weight-gradient path (A/B and parity tests)

extern "C" int rmcl_set_side_stream(void* stream) { g_side = (hipStream_t)stream; return 0; }

// ---- gradient-ready events of the last weight-gradient backward (overlapped data-parallel all-reduce) ----
static int g_grad_layers = 0;      // 0: no full backward has run
static bool g_grad_side = false;   // the weight gradients of that backward ran on the side stream
extern "C" int rmcl_grad_ready_wait(int layer, void* stream) {
  RMCL_REQUIRE(g_grad_layers > 0, "grad_ready_wait: no weight-gradient backward has been enqueued");
  RMCL_REQUIRE(layer >= 0 && layer < g_grad_layers && layer < 32, "grad_ready_wait: bad layer");
  HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, ev_slot(EV_MAIN_DONE, layer), 0));                 // dX chain + LayerNorm grads
  if (g_grad_side) HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, ev_slot(EV_SIDE_DONE, layer), 0));  // weight-gradient GEMMs
  return 0;
}

// one GEMM per (sample, head): element strides of A, B and C per sample (1) and per head (2)
static void per_head(GemmArgs& g, int B, int H, long sA1, long sA2, long sB1, long sB2, long sC1, long sC2) {
  g.nb1 = B; g.nb2 = H;
  g.sA1 = sA1; g.sA2 = sA2; g.sB1 = sB1; g.sB2 = sB2; g.sC1 = sC1; g.sC2 = sC2;
}

int rmcl_attention_fwd_impl(const void* qkv, const int* mask, void* out, void* probs, float* scores, int B, int N, int H, int dt,
                            int exact, hipStream_t s) {
  RMCL_REQUIRE(N >= 1 && N <= 512, "attention: N must be in 1..512");   // (before the score GEMM writes into the caller's buffers)
  // bf16 fast path: fused kernel; `probs` then holds only the per-row log-sum-exp (fp32 [B,H,NKP])
  if (dt == RMCL_BF16 && !exact && N <= 256) return rmcl_attn_fused_fwd(qkv, mask, out, (float*)probs, B, N, H, s);
  const int D = H * 64, ldp = ldp_of(N);
  const size_t e = esz(dt);
  // S = 0.125 * Q K^T   (batched over (b,h); Q/K rows are 3D apart, heads 64 apart)
  GemmArgs g = gemm_args(qkv, (const char*)qkv + (size_t)D * e, scores, N, N, 64, 3 * D, 3 * D, ldp);
  g.alpha = 0.125f;
  per_head(g, B, H, (long)N * 3 * D, 64, (long)N * 3 * D, 64, (long)H * N * ldp, (long)N * ldp);
  RMCL_TRY(rmcl_launch_gemm(g, dt, RMCL_F32, 1, 1, exact, s));
  RMCL_TRY(rmcl_softmax_fwd(scores, ldp, mask, probs, ldp, dt, B * H, N, H, s));
  // out[b*N+i, h*64+d] = sum_j P[b,h,i,j] V[b*N+j, 2D + h*64 + d]
  GemmArgs o = gemm_args(probs, (const char*)qkv + (size_t)2 * D * e, out, N, 64, N, ldp, 3 * D, D);
  per_head(o, B, H, (long)H * N * ldp, (long)N * ldp, (long)N * 3 * D, 64, (long)N * D, 64);
  RMCL_TRY(rmcl_launch_gemm(o, dt, dt, 1, 0, exact, s));
  return 0;
}

int rmcl_attention_bwd_impl(const void* qkv, const int* mask, const void* probs, const void* dout, const void* out, void* dqkv,
                            float* scores, void* dS, int B, int N, int H, int dt, int exact, hipStream_t s) {
  RMCL_REQUIRE(N >= 1 && N <= 512, "attention: N must be in 1..512");
  // bf16 fast path: probs = saved log-sum-exp, scores = scratch for delta (both fp32 [B,H,NKP]); with the forward's output
  // `out` (stashed in DATA and FULL mode) ONE kernel produces dQ, dK and dV
  if (dt == RMCL_BF16 && !exact && N <= 256)
    return rmcl_attn_fused_bwd(qkv, mask, dout, out, (const float*)probs, scores, dqkv, B, N, H, s);
  const int D = H * 64, ldp = ldp_of(N);
  const size_t e = esz(dt);
  const long sQ1 = (long)N * 3 * D, sP1 = (long)H * N * ldp, sP2 = (long)N * ldp;
  // dP = dO V^T
  GemmArgs g = gemm_args(dout, (const char*)qkv + (size_t)2 * D * e, scores, N, N, 64, D, 3 * D, ldp);
  per_head(g, B, H, (long)N * D, 64, sQ1, 64, sP1, sP2);
  RMCL_TRY(rmcl_launch_gemm(g, dt, RMCL_F32, 1, 1, exact, s));
  RMCL_TRY(rmcl_softmax_bwd(probs, ldp, scores, ldp, dS, ldp, dt, B * H, N, 0.125f, s));
  // dQ = dS K
  GemmArgs q = gemm_args(dS, (const char*)qkv + (size_t)D * e, dqkv, N, 64, N, ldp, 3 * D, 3 * D);
  per_head(q, B, H, sP1, sP2, sQ1, 64, sQ1, 64);
  RMCL_TRY(rmcl_launch_gemm(q, dt, dt, 1, 0, exact, s));
  // dK = dS^T Q
  GemmArgs k = gemm_args(dS, qkv, (char*)dqkv + (size_t)D * e, N, 64, N, ldp, 3 * D, 3 * D);
  per_head(k, B, H, sP1, sP2, sQ1, 64, sQ1, 64);
  RMCL_TRY(rmcl_launch_gemm(k, dt, dt, 0, 0, exact, s));
  // dV = P^T dO
  GemmArgs v = gemm_args(probs, dout, (char*)dqkv + (size_t)2 * D * e, N, 64, N, ldp, D, 3 * D);
  per_head(v, B, H, sP1, sP2, (long)N * D, 64, sQ1, 64);
  RMCL_TRY(rmcl_launch_gemm(v, dt, dt, 0, 0, exact, s));
  return 0;
}

extern "C" {

void rmcl_param_layout(const rmcl_dims* d, rmcl_layout* o) {
  int64_t off = 0;
  auto take = [&](int64_t n) { int64_t p = off; off += (n + 63) / 64 * 64; return p; };
  const int64_t D = d->D;
  o->word = take((int64_t)d->vocab * D);
  o->pos = take((int64_t)d->L * D);
  o->btype = take(2 * D);
  o->eln_w = take(D); o->eln_b = take(D);
  o->vtype = take((d->n_types == 3 ? 3 : 2) * D);     // NLVR2: [3, D] (the pre-training layout is unchanged otherwise)
  o->cls = take(D);
  o->pos_img = take((int64_t)((d->Pp > 0 ? d->Pp : d->P) + 1) * D);
  o->patch_w = take(D * d->patch_k);
  o->patch_b = take(D);
  o->layer0 = off;
  {
    int64_t base = off;
    o->ln1_w = take(D) - base; o->ln1_b = take(D) - base;
    o->qkv_w = take(3 * D * D) - base; o->qkv_b = take(3 * D) - base;
    o->proj_w = take(D * D) - base; o->proj_b = take(D) - base;
    o->ln2_w = take(D) - base; o->ln2_b = take(D) - base;
    o->fc1_w = take((int64_t)d->mlp * D) - base; o->fc1_b = take(d->mlp) - base;
    o->fc2_w = take((int64_t)d->mlp * D) - base; o->fc2_b = take(D) - base;
    o->layer_stride = off - base;
    off = base + o->layer_stride * d->layers;
  }
  o->norm_w = take(D); o->norm_b = take(D);
  o->mh0_w = take(D * D); o->mh0_b = take(D);
  o->mh1_w = take(D); o->mh1_b = take(D);
  o->mh3_w = take((int64_t)d->proj * D);
  o->ema_end = off;
  o->pool_w = take(D * D); o->pool_b = take(D);
  o->itm_w = take(2 * D); o->itm_b = take(64);
  o->total = off;
}

// (RMCL_MODE_STREAM_ATTN does not change the stash: the `probs` slots stay sized for the unfused matrices)
int64_t rmcl_stash_bytes(const rmcl_dims* d, int mode) { return (int64_t)carve_stash(*d, mode & ~RMCL_MODE_STREAM_ATTN, nullptr, nullptr) + 256; }
int64_t rmcl_workspace_bytes(const rmcl_dims* d) { return (int64_t)carve_work(*d, nullptr, nullptr) + 256; }

// rank != NULL: the image tokens and their mask come from a cache of rmcl_visual_embed outputs (rmcl_encoder_forward_rank); `patches`
// and `ragged` are then unused
static int encoder_forward_impl(const rmcl_dims* d, int mode, const float* params32, const void* params_lp, const int64_t* text_ids,
                                const int64_t* text_mask, const void* patches, int32_t* co_mask, void* stash, void* workspace,
                                float* xn, uint32_t drop_seed, float drop_p, const rmcl_ragged* ragged, const rmcl_fold* fold,
                                const rmcl_rank_src* rank, const int32_t* replaced, int64_t mask_token_off, void* stream) {
  RMCL_TRY(check_dims(d));
  RMCL_REQUIRE(!ragged || (ragged->sel && ragged->counts && ragged->hw && ragged->pos_tok), "encoder_forward: incomplete rmcl_ragged");
  RMCL_REQUIRE(rank || ragged || d->Pp == 0 || d->Pp == d->P, "encoder_forward: P != Pp needs the rmcl_ragged selection");
  RMCL_REQUIRE(params32 && text_ids && text_mask && (patches || rank) && co_mask && workspace && xn, "encoder_forward: NULL argument");
  RMCL_REQUIRE(d->dtype == RMCL_F32 || params_lp, "encoder_forward: bf16 mode needs the bf16 shadow arena");
  const bool tail_req = (mode & RMCL_MODE_CLS_TAIL) != 0;     // only the cls rows of xn will be read (include/rmcl.h)
  const bool streamed = stream_attn(*d, mode);                // attention through the streaming kernels (include/rmcl.h)
  mode &= ~(RMCL_MODE_CLS_TAIL | RMCL_MODE_STREAM_ATTN);
  RMCL_REQUIRE(mode == RMCL_MODE_INFER || stash, "encoder_forward: stash required unless mode is INFER");
  RMCL_REQUIRE(!tail_req || d->B <= 1024, "encoder_forward: the cls-only tail needs B <= 1024");
  Ctx c{*d, params32, params_lp, {}, (hipStream_t)stream, d->dtype};
  rmcl_param_layout(d, &c.lay);
  const rmcl_layout& y = c.lay;
  Stash st{};
  Work w{};
  carve_stash(*d, mode, stash, &st);
  carve_work(*d, workspace, &w);
  const int B = d->B, L = d->L, P = d->P, N = L + 1 + P, D = d->D, M = B * N, dt = d->dtype;
  const bool keep = mode != RMCL_MODE_INFER, full = mode == RMCL_MODE_FULL;
  hipStream_t s = c.s;
  Dropout drop{};
  RMCL_TRY(make_dropout(drop_seed, drop_p, true, &drop));

  float* x0 = keep ? st.layer[0].x_in : w.x_a;
  RMCL_TRY(rmcl_text_embed_fwd((const long*)text_ids, c.V(y.word), c.V(y.pos), c.V(y.btype), c.V(y.eln_w), c.V(y.eln_b),
                               c.V(y.vtype), 1e-12f, x0, keep ? st.text_e : nullptr, keep ? st.text_mean : nullptr,
                               keep ? st.text_rstd : nullptr, B, L, N, D, drop.site(0, DROP_SITE_TEXT), drop.thresh, drop.inv_keep, s));
  if (rank) {
    RMCL_TRY(rmcl_rank_assemble(rank->embeds, rank->masks, rank->img_of, rank->n_img, rank->ld_tok, (const long*)text_mask, c.V(y.vtype) + D,
                                x0, co_mask, B, P, L, N, D, s));
  } else {
    // the pixel path: patch rows, (resized) position rows, cls + token type, mask from the patch rows
    RMCL_TRY(patch_embed(c, w, patches, replaced, mask_token_off, ragged));
    // image token type (vilt_module.py:315-321): row 1, row 2 (img_type 2), or row 1 + (b & 1) per pair (img_type -1)
    RMCL_TRY(rmcl_image_assemble_fwd(w.pe, c.V(y.cls), ragged ? ragged->pos_tok : c.V(y.pos_img), c.V(y.vtype) + (d->img_type == 2 ? 2 : 1) * D,
                                     x0, B, P, L, N, D, drop.site(0, DROP_SITE_IMAGE), drop.thresh, drop.inv_keep, ragged ? 1 : 0,
                                     d->img_type == -1 ? 1 : 0, s));
    RMCL_TRY(rmcl_co_mask((const long*)text_mask, patches, dt, co_mask, B, L, P, 3, d->patch_k / 3, s));
  }

  FwdPass pass{c, w, st, fold, M, D, d->mlp, keep, full, /*folded, centred, tiled, probe: decided below*/ false, false, false, false, drop};
  // LayerNorm folded into the consuming GEMMs (gemm.h EPI_LNFOLD / EPI_ROWSTAT): passes that keep no LayerNorm output
  // (INFER, DATA), bf16, dropout off, and only where every GEMM involved runs on the 192-row tile kernels
  // (dropout: the 192-row tile kernels carry the dropout epilogues as separate instantiations since round 4, so the fold stays on)
  pass.folded = fold && fold->wf && fold->sc && !full && dt == RMCL_BF16 && !d->exact && D % 192 == 0;
  if (pass.folded) {
    const FwdPass q = pass.as_probe(true, false);
    const FwdLayer b = q.layer(0, w.x_a);
    pass.folded = rmcl_gemm_routes_to_tile192(q.qkv(0, b), 1, 1) && rmcl_gemm_routes_to_tile192(q.fc1(0, b), 1, 1) &&
                  rmcl_gemm_routes_to_tile192(q.proj(0, b), 1, 1) && rmcl_gemm_routes_to_tile192(q.fc2(0, b), 1, 1);
  }
  // Tiled pre-activation stash (gemm.h EPI_PREACT_TILED): decided ONCE per pass - both the pass's fc1 form and the backward's fc2-dX
  // (transposed weight shadows, [cols][K]) must go to the 192x384 kernel with the flag - and recorded with the stash: the backward
  // reads the record.  (The cls-only tail's compact fp32 u_c of the last layer is not a GEMM stash of this kind and stays as it is.)
  // (and the attention must leave the tail of the `probs` slots to the tiled buffer, carve_stash: the fused kernels, N <= 256, or the streamed ones)
  pass.tiled = g_preact_tiled && keep && dt == RMCL_BF16 && !d->exact && (N <= 256 || streamed) && st.layer[0].u_t != nullptr;
  if (pass.tiled) {
    const FwdPass q = pass.as_probe(pass.folded, true);
    const GemmArgs p1 = q.fc1(0, q.layer(0, w.x_a));
    // the backward's fc2-dX on its workspace buffers; the forward has no transposed shadows, the shadow arena stands in for them (same layout offsets)
    const GemmArgs p2 = BwdSites{c, M, c.Plp, true, drop}.fc2(0, w.dxT, w.u, w.du);
    pass.tiled = rmcl_gemm_fast_takes(p1, RMCL_BF16, RMCL_BF16, 1, 1) && rmcl_gemm_fast_takes(p2, RMCL_BF16, RMCL_BF16, 1, 1) &&
                 rmcl_gemm_route_code(p1, RMCL_BF16, 1, 1) == 2 && rmcl_gemm_route_code(p2, RMCL_BF16, 1, 1) == 2;
  }
  if (keep) note_stash(stash, streamed, pass.tiled);
  // shift-robust form of the fold (gemm.h ln_center): every producer stores bf16(x - c) and the partial sums of (x - c), c = the row mean
  // of the row's PREVIOUS LayerNorm (LN is shift-invariant: exact for any c), so the operand's rounding follows the row's spread instead of
  // its offset.  rmcl_tune_set(11, 0) restores the uncentred round-2 form (A/B, precision tests).
  pass.centred = pass.folded && rmcl_lnfold_centred();
  float* x = x0;
  for (int l = 0; l < d->layers; ++l) {
    const FwdLayer b = pass.layer(l, x);
    // (a folded pass: layer 0's qkv still reads the embedding through the LayerNorm kernel; later layers read the previous fc2's bf16 copy)
    if (!(pass.folded && l > 0))
      RMCL_TRY(rmcl_ln_fwd(x, D, c.V(c.L(l, y.ln1_w)), c.V(c.L(l, y.ln1_b)), 1e-6f, b.ln1, D, dt, b.mean1, b.rstd1, M, D, 0, s));
    RMCL_TRY(gemm(c, pass.qkv(l, b), dt, dt, 1, 1));
    if (streamed) RMCL_TRY(rmcl_attn_stream_fwd(b.qkv, co_mask, b.ao, (float*)b.probs, B, N, d->H, s));   // `probs` keeps the log-sum-exp
    else RMCL_TRY(rmcl_attention_fwd_impl(b.qkv, co_mask, b.ao, b.probs, w.scores, B, N, d->H, dt, d->exact, s));
    if (tail_req && l + 1 == d->layers) return forward_tail(pass, l, b, xn);
    RMCL_TRY(gemm(c, pass.proj(l, b), dt, RMCL_F32, 1, 1));
    if (!pass.folded)
      RMCL_TRY(rmcl_ln_fwd(b.x_mid, D, c.V(c.L(l, y.ln2_w)), c.V(c.L(l, y.ln2_b)), 1e-6f, b.ln2, D, dt, b.mean2, b.rstd2, M, D, 0, s));
    RMCL_TRY(gemm(c, pass.fc1(l, b), dt, dt, 1, 1));
    RMCL_TRY(gemm(c, pass.fc2(l, b), dt, RMCL_F32, 1, 1));
    x = b.x_out;
  }
  RMCL_TRY(rmcl_ln_fwd(x, D, c.V(y.norm_w), c.V(y.norm_b), 1e-6f, xn, D, RMCL_F32, keep ? st.meanF : w.stat,
                       keep ? st.rstdF : w.stat + M, M, D, 0, s));
  return 0;
}

int rmcl_encoder_forward(const rmcl_dims* d, int mode, const float* params32, const void* params_lp, const int64_t* text_ids,
                         const int64_t* text_mask, const void* patches, int32_t* co_mask, void* stash, void* workspace,
                         float* xn, uint32_t drop_seed, float drop_p, const rmcl_ragged* ragged, const rmcl_fold* fold, void* stream) {
  return encoder_forward_impl(d, mode, params32, params_lp, text_ids, text_mask, patches, co_mask, stash, workspace, xn, drop_seed, drop_p,
                              ragged, fold, nullptr, nullptr, 0, stream);
}

int rmcl_encoder_forward_mpp(const rmcl_dims* d, int mode, const float* params32, const void* params_lp, const int64_t* text_ids,
                             const int64_t* text_mask, const void* patches, int32_t* co_mask, void* stash, void* workspace, float* xn,
                             uint32_t drop_seed, float drop_p, const rmcl_ragged* ragged, const rmcl_fold* fold, const int32_t* replaced,
                             int64_t mask_token_off, void* stream) {
  RMCL_REQUIRE(!(mode & RMCL_MODE_CLS_TAIL), "encoder_forward_mpp: no cls-only tail (the loss reads the image rows)");
  RMCL_REQUIRE(!replaced || (d && mask_token_off >= 0 && mask_token_off % 4 == 0), "encoder_forward_mpp: bad mask_token offset");
  return encoder_forward_impl(d, mode, params32, params_lp, text_ids, text_mask, patches, co_mask, stash, workspace, xn, drop_seed, drop_p,
                              ragged, fold, nullptr, replaced, mask_token_off, stream);
}

int rmcl_encoder_forward_rank(const rmcl_dims* d, int mode, const float* params32, const void* params_lp, const int64_t* text_ids,
                              const int64_t* text_mask, const rmcl_rank_src* src, int32_t* co_mask, void* workspace, float* xn,
                              const rmcl_fold* fold, void* stream) {
  RMCL_REQUIRE(d && src && src->embeds && src->masks && src->img_of, "encoder_forward_rank: NULL argument");
  RMCL_REQUIRE((mode & ~(RMCL_MODE_CLS_TAIL | RMCL_MODE_STREAM_ATTN)) == RMCL_MODE_INFER, "encoder_forward_rank: INFER mode only (the rank pass keeps no stash)");
  RMCL_REQUIRE(src->n_img >= 1 && d->P >= 1 && d->P + 1 <= src->ld_tok, "encoder_forward_rank: the cache slots hold fewer than 1 + P token rows");
  RMCL_REQUIRE(d->img_type == 0 || d->img_type == 1, "encoder_forward_rank: image tokens take token-type row 1");
  return encoder_forward_impl(d, mode, params32, params_lp, text_ids, text_mask, nullptr, co_mask, nullptr, workspace, xn, 0u, 0.f, nullptr,
                              fold, src, nullptr, 0, stream);
}

}  // extern "C"

static int visual_embed_impl(const rmcl_dims* d, const float* params32, const void* params_lp, const void* patches, const rmcl_ragged* ragged,
                             void* workspace, float* out, int32_t* masks, const int32_t* replaced, int64_t mask_token_off, void* stream) {
  RMCL_TRY(check_dims(d));
  RMCL_REQUIRE(params32 && patches && workspace && out && masks, "visual_embed: NULL argument");
  RMCL_REQUIRE(!ragged || (ragged->sel && ragged->counts && ragged->hw && ragged->pos_tok), "visual_embed: incomplete rmcl_ragged");
  RMCL_REQUIRE(ragged || d->Pp == 0 || d->Pp == d->P, "visual_embed: P != Pp needs the rmcl_ragged selection");
  RMCL_REQUIRE(d->dtype == RMCL_F32 || params_lp, "visual_embed: bf16 mode needs the bf16 shadow arena");
  Ctx c{*d, params32, params_lp, {}, (hipStream_t)stream, d->dtype};
  rmcl_param_layout(d, &c.lay);
  const rmcl_layout& y = c.lay;
  Work w{};
  carve_work(*d, workspace, &w);
  const int B = d->B, P = d->P, D = d->D;
  RMCL_TRY(patch_embed(c, w, patches, replaced, mask_token_off, ragged));
  RMCL_TRY(rmcl_visual_assemble(w.pe, c.V(y.cls), ragged ? ragged->pos_tok : c.V(y.pos_img), ragged ? 1 : 0, out, B, P, D, c.s));
  // the mask of rmcl_encoder_forward's image tokens (L = 0: no text columns; the text-mask pointer is never read)
  RMCL_TRY(rmcl_co_mask(nullptr, patches, d->dtype, masks, B, 0, P, 3, d->patch_k / 3, c.s));
  return 0;
}

extern "C" {

int rmcl_visual_embed(const rmcl_dims* d, const float* params32, const void* params_lp, const void* patches, const rmcl_ragged* ragged,
                      void* workspace, float* out, int32_t* masks, void* stream) {
  return visual_embed_impl(d, params32, params_lp, patches, ragged, workspace, out, masks, nullptr, 0, stream);
}

int rmcl_visual_embed_mpp(const rmcl_dims* d, const float* params32, const void* params_lp, const void* patches, const rmcl_ragged* ragged,
                          void* workspace, float* out, int32_t* masks, const int32_t* replaced, int64_t mask_token_off, void* stream) {
  RMCL_REQUIRE(!replaced || (mask_token_off >= 0 && mask_token_off % 4 == 0), "visual_embed_mpp: bad mask_token offset");
  return visual_embed_impl(d, params32, params_lp, patches, ragged, workspace, out, masks, replaced, mask_token_off, stream);
}

}  // extern "C"

// replaced != NULL: the forward substituted the mask token (rmcl_encoder_backward_mpp)
static int encoder_backward_impl(const rmcl_dims* d, int mode, const float* params32, const void* params_lp, const int64_t* text_ids,
                                 const void* patches, const int32_t* co_mask, void* stash, void* workspace, const float* dxn,
                                 int cls_only, void* dpatches, float* dtext, float* G, uint32_t drop_seed, float drop_p,
                                 const rmcl_ragged* ragged, const void* params_lpT, const int32_t* replaced, int64_t mask_token_off,
                                 void* stream) {
  RMCL_TRY(check_dims(d));
  const bool streamed = stream_attn(*d, mode);
  mode &= ~RMCL_MODE_STREAM_ATTN;
  RMCL_REQUIRE(!ragged || mode != RMCL_MODE_FULL || ragged->dpos_tok, "encoder_backward: rmcl_ragged.dpos_tok needed in FULL mode");
  RMCL_REQUIRE(mode == RMCL_MODE_DATA || mode == RMCL_MODE_FULL, "encoder_backward: mode must be DATA or FULL");
  RMCL_REQUIRE(params32 && stash && workspace && dxn && co_mask, "encoder_backward: NULL argument");
  StashNote note{};
  const bool noted = stash_note(stash, &note);                 // (a stash the table no longer knows: nothing to compare the attention setting with)
  RMCL_REQUIRE(!noted || note.stream == streamed, "encoder_backward: RMCL_MODE_STREAM_ATTN differs from the forward that filled this stash");
  RMCL_REQUIRE(mode != RMCL_MODE_FULL || (G && text_ids && patches), "encoder_backward: FULL mode needs grads32, text_ids, patches");
  // layout of the `u` slots: what the forward that filled this stash recorded
  const int u_tiled = d->dtype == RMCL_BF16 && !d->exact ? (noted ? (note.tiled ? 1 : 0) : -1) : 0;
  RMCL_REQUIRE(u_tiled >= 0, "encoder_backward: no forward on record for this stash (the layout of its pre-activation slots is unknown)");
  RMCL_REQUIRE(!u_tiled || (d->L + 1 + d->P <= 256 || streamed), "encoder_backward: a tiled pre-activation stash goes with fused or streamed attention");
  RMCL_REQUIRE(!u_tiled || params_lpT, "encoder_backward: this stash holds the tiled pre-activation (rmcl_tune_set key 15), whose backward needs the "
                                       "transposed weight shadows params_lpT");
  RMCL_REQUIRE(d->dtype == RMCL_F32 || params_lp, "encoder_backward: bf16 mode needs the bf16 shadow arena");
  Ctx c{*d, params32, params_lp, {}, (hipStream_t)stream, d->dtype};
  rmcl_param_layout(d, &c.lay);
  const rmcl_layout& y = c.lay;
  Stash st{};
  Work w{};
  carve_stash(*d, mode, stash, &st);
  carve_work(*d, workspace, &w);
  const int B = d->B, L = d->L, P = d->P, N = L + 1 + P, D = d->D, M = B * N, dt = d->dtype, mlp = d->mlp;
  const bool full = mode == RMCL_MODE_FULL;
  hipStream_t s = c.s;
  auto Gp = [&](int64_t off) { return G + off; };

  // final LayerNorm backward -> dx (the residual-stream gradient, fp32)
  const float* dy = dxn;
  const bool tail = cls_only == 2;               // the forward of this stash used the cls-only tail (compact last-layer rows)
  RMCL_REQUIRE(!tail || d->B <= 1024, "encoder_backward: the cls-only tail needs B <= 1024");
  if (cls_only && !tail) {
    HIP_TRY(hipMemsetAsync(w.dxn_full, 0, (size_t)M * D * sizeof(float), s));
    RMCL_TRY(rmcl_scatter_rows(dxn, w.dxn_full, B, D, 1, N, 0, 0, s));
    dy = w.dxn_full;
  }
  // bf16 copy of dx written by every LN backward (ping-pong T[0]/T[1]); with a side stream the weight
  // gradients of layer l run concurrently with the data-gradient chain, reading the copy the chain no
  // longer writes (events order the reuse of T / du / dqkv two sub-layers later).
  Dropout drop{};
  RMCL_TRY(make_dropout(drop_seed, drop_p, false, &drop));
  const bool lpm = dt != RMCL_F32 || drop.thresh != 0;      // a (masked) copy of dx in the GEMM operand type is needed
  // transposed bf16 weight shadows: dX = dY W as [rows][K] x [cols][K] (BwdSites::lpT)
  const bool WT = params_lpT != nullptr && dt == RMCL_BF16 && !d->exact;
  const BwdSites sites{c, M, WT ? params_lpT : nullptr, u_tiled != 0, drop};
  // GROUPED weight gradients (bf16 fast path at the step's shapes): ONE launch per layer computes the four dW, the four bias
  // gradients and finishes the layer's LayerNorm dgamma/dbeta (gemm_dw_group_kernel); otherwise four split-K GEMMs + slab
  // reduces + column sums per layer.
  const int Lr = d->layers;
  const bool grouped = full && dt == RMCL_BF16 && !d->exact && M % 64 == 0 && M >= 256 && D % 768 == 0 && mlp % 768 == 0 &&
                       2 * Lr + 1 <= 64 && rmcl_gemm_fast_get_cfg() != 2 && g_dw_grouped;
  const bool use_side = full && lpm && g_side != nullptr;
  if (use_side || full) RMCL_TRY(ensure_events());
  // copies of dx in the operand type, written by every LN backward.  Legacy path: ping-pong T[0]/T[1] (with a side stream the
  // weight gradients of layer l read the copy the chain no longer writes).  Grouped path: rotation over three copies - layer l
  // reads T[ia] (fc2) and T[ib] (proj) in its one weight-gradient launch while LN backward 1 already writes T[ic] for layer l-1.
  void* T[3] = {lpm ? w.dxT : nullptr, lpm ? ((use_side || grouped) ? w.dxT2 : w.dxT) : nullptr, lpm ? w.dxT3 : nullptr};
  void* DU[2] = {w.du, (use_side || grouped) ? w.du2 : w.du};
  void* DQ[2] = {w.dqkv, (use_side || grouped) ? w.dqkv2 : w.dqkv};
  Ctx cs{c.d, c.P32, c.Plp, c.lay, use_side ? g_side : c.s, c.dt};      // where the weight gradients run
  auto rep_slot = [&](int idx) { return grouped ? w.ln_rep + (size_t)idx * RMCL_LN_REP_FLOATS : nullptr; };   // 0: final norm, 1+2l: ln2, 2+2l: ln1
  if (grouped) HIP_TRY(hipMemsetAsync(w.ln_rep, 0, (size_t)(2 * Lr + 1) * RMCL_LN_REP_FLOATS * sizeof(float), s));
  // stash prefetch: while layer l's backward runs, the idle CUs touch layer l - 1's cold operands into the Infinity Cache
  const bool pref = g_prefetch_mask != 0 && g_pref != nullptr && dt == RMCL_BF16 && !d->exact && M >= 4096;
  if (pref)
    for (; g_npev < 64; ++g_npev) HIP_TRY(hipEventCreateWithFlags(&g_pev[g_npev], hipEventDisableTiming));
  static int pev_rot = 0;
  auto prefetch_layer = [&](int l) -> int {
    if (!pref || l < 0) return 0;
    const LayerStash& q = st.layer[l];
    hipEvent_t ev = g_pev[(pev_rot++) & 63];
    HIP_TRY(hipEventRecord(ev, s));
    HIP_TRY(hipStreamWaitEvent(g_pref, ev, 0));
    const size_t e2 = esz(dt);
    if (g_prefetch_mask & 1) RMCL_TRY(rmcl_touch(q.u, (size_t)M * mlp * e2, g_prefetch_wgs, g_pref));
    if (g_prefetch_mask & 2) {
      RMCL_TRY(rmcl_touch(q.qkv, (size_t)M * 3 * D * e2, g_prefetch_wgs, g_pref));
      RMCL_TRY(rmcl_touch(q.ao, (size_t)M * D * e2, g_prefetch_wgs, g_pref));
    }
    if (g_prefetch_mask & 4) {
      RMCL_TRY(rmcl_touch(q.x_mid, (size_t)M * D * 4, g_prefetch_wgs, g_pref));
      RMCL_TRY(rmcl_touch(q.x_in, (size_t)M * D * 4, g_prefetch_wgs, g_pref));
    }
    return 0;
  };
  int cur = 0;
  float* dxc = w.dxn_full;                       // tail: gradient of the B cls rows [B, D] f32
  if (tail) {
    // forward ran with RMCL_MODE_CLS_TAIL: final LayerNorm backward on the B compact rows
    RMCL_TRY(rmcl_ln_bwd(dxn, D, RMCL_F32, st.x_final, D, st.meanF, st.rstdF, c.V(y.norm_w), c.V(y.norm_b), dxc, D, 0,
                         full ? Gp(y.norm_w) : nullptr, full ? Gp(y.norm_b) : nullptr, B, D, 0, s));
  } else {
    RMCL_TRY(rmcl_ln_bwd_lp(dy, D, RMCL_F32, st.x_final, D, st.meanF, st.rstdF, c.V(y.norm_w), c.V(y.norm_b), w.dx, D, 0,
                            full ? Gp(y.norm_w) : nullptr, full ? Gp(y.norm_b) : nullptr, M, D, 0, T[0], dt,
                            drop.site(d->layers - 1, DROP_SITE_FC2), drop.thresh, drop.inv_keep, rep_slot(0), s));
  }
  // gradient w.r.t. the LayerNorm outputs (dX GEMM -> LN backward): in the operand dtype, like du / dqkv / dao (bf16 mode
  // halves the 36 MB write + read per LayerNorm); fp32 mode is unchanged
  const int dln_dt = lpm ? dt : RMCL_F32;
  for (int l = Lr - 1; l >= 0; --l) {
    const LayerStash& ls = st.layer[l];
    RMCL_TRY(prefetch_layer(l - 1));
    void* du = DU[l & 1];
    void* dqkv = DQ[l & 1];
    const int ia = cur, ib = grouped ? (cur + 1) % 3 : cur ^ 1, ic = grouped ? (cur + 2) % 3 : cur;
    const bool tail_l = tail && l == Lr - 1;
    const bool per_gemm = full && !grouped;      // the layer's weight gradients as separate GEMMs (on the side stream when there is one)
    const void* dxT = lpm ? T[ia] : (const void*)w.dx;
    const void* dxT_b = lpm ? T[ib] : (const void*)w.dx;
    auto dw = [&](const void* dY, const void* X, int64_t w_rel, int64_t b_rel, int Nout, int Kin) {
      return linear_dw(cs, w, dY, X, Gp(c.L(l, w_rel)), Gp(c.L(l, b_rel)), Nout, Kin, M);
    };
    auto dw_qkv = [&] { return dw(dqkv, ls.ln1, y.qkv_w, y.qkv_b, 3 * D, D); };
    if (tail_l) {
      RMCL_TRY(backward_tail(c, w, ls, l, full ? G : nullptr, drop, dxc));
      if (per_gemm && use_side) HIP_TRY(hipEventRecord(ev_slot(EV_MLP_DONE, l), cs.s));   // (no MLP weight-gradient work on the side stream)
    } else {
      // ---- MLP ----
      if (use_side && !grouped && l + 2 < Lr) HIP_TRY(hipStreamWaitEvent(s, ev_slot(EV_MLP_DONE, l + 2), 0));   // du buffer free again
      RMCL_TRY(gemm(c, sites.fc2(l, dxT, u_tiled ? ls.u_t : ls.u, du), dt, dt, 1, sites.b_kc()));
      if (per_gemm) {
        if (use_side) { HIP_TRY(hipEventRecord(ev_slot(EV_FORK, 2 * l), s)); HIP_TRY(hipStreamWaitEvent(cs.s, ev_slot(EV_FORK, 2 * l), 0)); }
        RMCL_TRY(dw(dxT, ls.h, y.fc2_w, y.fc2_b, D, mlp));
        RMCL_TRY(dw(du, ls.ln2, y.fc1_w, y.fc1_b, mlp, D));
        if (use_side) HIP_TRY(hipEventRecord(ev_slot(EV_MLP_DONE, l), cs.s));
      }
      RMCL_TRY(gemm(c, sites.fc1(l, du, w.dln), dt, dln_dt, 1, sites.b_kc()));
      if (use_side && l + 1 < Lr) HIP_TRY(hipStreamWaitEvent(s, ev_slot(EV_SIDE_DONE, l + 1), 0));   // T[ib] free again (grouped: layer l+1's whole
                                                                                                     // weight-gradient launch has finished)
      RMCL_TRY(rmcl_ln_bwd_lp(w.dln, D, dln_dt, ls.x_mid, D, ls.mean2, ls.rstd2, c.V(c.L(l, y.ln2_w)), c.V(c.L(l, y.ln2_b)), w.dx, D, 1,
                              full ? Gp(c.L(l, y.ln2_w)) : nullptr, full ? Gp(c.L(l, y.ln2_b)) : nullptr, M, D, 0, T[ib], dt,
                              drop.site(l, DROP_SITE_PROJ), drop.thresh, drop.inv_keep, rep_slot(1 + 2 * l), s));
      // ---- attention ----
      RMCL_TRY(gemm(c, sites.proj(l, dxT_b, w.dao), dt, dt, 1, sites.b_kc()));
    }
    if (use_side && !grouped && l + 2 < Lr) HIP_TRY(hipStreamWaitEvent(s, ev_slot(EV_SIDE_DONE, l + 2), 0));   // dqkv buffer free again
    if (streamed) RMCL_TRY(rmcl_attn_stream_bwd(ls.qkv, co_mask, w.dao, ls.ao, (const float*)ls.probs, w.scores, dqkv, B, N, d->H, s));
    else RMCL_TRY(rmcl_attention_bwd_impl(ls.qkv, co_mask, ls.probs, w.dao, ls.ao, dqkv, w.scores, w.dS, B, N, d->H, dt, d->exact, s));
    if (per_gemm) {
      if (use_side) { HIP_TRY(hipEventRecord(ev_slot(EV_FORK, 2 * l + 1), s)); HIP_TRY(hipStreamWaitEvent(cs.s, ev_slot(EV_FORK, 2 * l + 1), 0)); }
      if (!tail_l) RMCL_TRY(dw(dxT_b, ls.ao, y.proj_w, y.proj_b, D, D));
      RMCL_TRY(dw_qkv());
      if (use_side) HIP_TRY(hipEventRecord(ev_slot(EV_SIDE_DONE, l), cs.s));
    }
    RMCL_TRY(gemm(c, sites.qkv(l, dqkv, w.dln), dt, dln_dt, 1, sites.b_kc()));
    if (use_side && !grouped) HIP_TRY(hipStreamWaitEvent(s, ev_slot(EV_MLP_DONE, l), 0));             // T[ic] free again
    RMCL_TRY(rmcl_ln_bwd_lp(w.dln, D, dln_dt, ls.x_in, D, ls.mean1, ls.rstd1, c.V(c.L(l, y.ln1_w)), c.V(c.L(l, y.ln1_b)), w.dx, D, 1,
                            full ? Gp(c.L(l, y.ln1_w)) : nullptr, full ? Gp(c.L(l, y.ln1_b)) : nullptr, M, D, 0, T[ic], dt,
                            drop.site(l - 1, DROP_SITE_FC2), l > 0 ? drop.thresh : 0u, drop.inv_keep, tail_l ? nullptr : rep_slot(2 + 2 * l), s));
    cur = ic;
    // EV_MAIN_DONE: everything of layer l that runs on the main stream is enqueued (with the grouped launch on the SAME stream that
    // includes the launch, recorded below)
    if (full && (use_side || !grouped)) HIP_TRY(hipEventRecord(ev_slot(EV_MAIN_DONE, l), s));
    if (grouped) {
      // everything the layer's weight gradients read is final: both dx copies, du, dqkv, the stash, the LN replicas
      if (use_side) HIP_TRY(hipStreamWaitEvent(cs.s, ev_slot(EV_MAIN_DONE, l), 0));
      if (tail_l) {
        // tail layer: fc2 / fc1 / proj gradients were formed from the B cls rows (backward_tail); only qkv reduces over all tokens
        RMCL_TRY(dw_qkv());
      } else {
        DwGroupArgs a{};
        const void* As[4] = {dxT, du, dxT_b, dqkv};                                          // dY of fc2, fc1, proj, qkv
        const void* Bs[4] = {ls.h, ls.ln2, ls.ao, ls.ln1};                                   // their inputs X
        const int64_t wo[4] = {y.fc2_w, y.fc1_w, y.proj_w, y.qkv_w}, bo[4] = {y.fc2_b, y.fc1_b, y.proj_b, y.qkv_b};
        const int nout[4] = {D, mlp, D, 3 * D}, kin[4] = {mlp, D, D, D};
        a.tile_base[0] = 0;
        for (int q = 0; q < 4; ++q) {
          a.A[q] = (const unsigned short*)As[q]; a.B[q] = (const unsigned short*)Bs[q];
          a.C[q] = Gp(c.L(l, wo[q])); a.bias[q] = Gp(c.L(l, bo[q]));
          a.lda[q] = nout[q]; a.ldb[q] = kin[q]; a.ldc[q] = kin[q]; a.tiles_n[q] = kin[q] / 192;
          a.tile_base[q + 1] = a.tile_base[q] + (nout[q] / 192) * (kin[q] / 192);
        }
        a.K = M;
        a.rep = w.ln_rep; a.G = G; a.D = D;
        a.nslots = 0;
        auto add_slot = [&](int idx, int64_t gw, int64_t gb) { a.slot[a.nslots] = idx; a.g_gamma[a.nslots] = gw; a.g_beta[a.nslots] = gb; ++a.nslots; };
        add_slot(1 + 2 * l, c.L(l, y.ln2_w), c.L(l, y.ln2_b));
        add_slot(2 + 2 * l, c.L(l, y.ln1_w), c.L(l, y.ln1_b));
        if (l == Lr - 1) add_slot(0, y.norm_w, y.norm_b);
        RMCL_TRY(rmcl_launch_dw_group(a, cs.s));
      }
      HIP_TRY(hipEventRecord(ev_slot(use_side ? EV_SIDE_DONE : EV_MAIN_DONE, l), cs.s));
    }
  }
  if (full) { g_grad_layers = Lr; g_grad_side = use_side; }
  if (use_side) HIP_TRY(hipStreamWaitEvent(s, ev_slot(EV_SIDE_DONE, 0), 0));                 // join: all side work done

  // ---- embeddings ----
  RMCL_TRY(rmcl_image_assemble_bwd(w.dx, w.dpe, dt, full ? Gp(y.pos_img) : nullptr, full ? Gp(y.cls) : nullptr,
                                   full ? Gp(y.vtype) + (d->img_type == 2 ? 2 : 1) * D : nullptr, B, P, L, N, D,
                                   drop.site(0, DROP_SITE_IMAGE), drop.thresh, drop.inv_keep, (ragged && full) ? ragged->dpos_tok : nullptr,
                                   d->img_type == -1 ? 1 : 0, s));
  // the replaced patches' gradient goes to the mask token; their dpe rows are zeroed BEFORE dpatches, the patch-weight gradient and the
  // patch-bias column sum read them
  if (replaced)
    RMCL_TRY(rmcl_mask_token_bwd(w.dx, w.dpe, dt, replaced, full ? Gp(mask_token_off) : nullptr, w.dln /* free until the text rows */, B, P, L, N, D,
                                 drop.site(0, DROP_SITE_IMAGE), drop.thresh, drop.inv_keep, s));
  if (ragged && full)                                          // position-table gradient through the per-sample resize
    RMCL_TRY(rmcl_pos_resize_bwd(ragged->dpos_tok, ragged->sel, ragged->counts, ragged->hw, ragged->sel_ld, ragged->gw, ragged->G0, B, P, D,
                                 Gp(y.pos_img), s));
  if (dpatches) {
    GemmArgs g = gemm_args(w.dpe, c.W(y.patch_w), dpatches, B * P, d->patch_k, D, D, d->patch_k, d->patch_k);
    RMCL_TRY(gemm(c, g, dt, dt, 1, 0));
  }
  if (full) RMCL_TRY(linear_dw(c, w, w.dpe, patches, Gp(y.patch_w), Gp(y.patch_b), D, d->patch_k, B * P));
  if (full || dtext) {
    // text rows: x[b*N+t] = LN(e) + vtype[0];  de = gradient wrt the embedding sum e, i.e. wrt the output of
    // word_embeddings (the tensor the reference's saliency hook captures, greedy_attack_vilt.py:414-452)
    float* de = dtext ? dtext : w.de;
    RMCL_TRY(rmcl_gather_rows(w.dx, w.dln, B * L, D, L, N, 0, s));
    if (full) RMCL_TRY(rmcl_colsum(w.dln, D, RMCL_F32, Gp(y.vtype), B * L, D, s));
    RMCL_TRY(rmcl_dropout_apply(w.dln, (long)B * L * D, drop.site(0, DROP_SITE_TEXT), drop.thresh, drop.inv_keep, s));
    RMCL_TRY(rmcl_ln_bwd(w.dln, D, RMCL_F32, st.text_e, D, st.text_mean, st.text_rstd, c.V(y.eln_w), c.V(y.eln_b), de, D, 0,
                         full ? Gp(y.eln_w) : nullptr, full ? Gp(y.eln_b) : nullptr, B * L, D, 0, s));
    if (full) RMCL_TRY(rmcl_text_embed_scatter((const long*)text_ids, de, Gp(y.word), Gp(y.pos), Gp(y.btype), B, L, D, 0, s));
  }
  return 0;
}

extern "C" {

int rmcl_encoder_backward(const rmcl_dims* d, int mode, const float* params32, const void* params_lp, const int64_t* text_ids,
                          const void* patches, const int32_t* co_mask, void* stash, void* workspace, const float* dxn,
                          int cls_only, void* dpatches, float* dtext, float* G, uint32_t drop_seed, float drop_p,
                          const rmcl_ragged* ragged, const void* params_lpT, void* stream) {
  return encoder_backward_impl(d, mode, params32, params_lp, text_ids, patches, co_mask, stash, workspace, dxn, cls_only, dpatches, dtext, G,
                               drop_seed, drop_p, ragged, params_lpT, nullptr, 0, stream);
}

int rmcl_encoder_backward_mpp(const rmcl_dims* d, int mode, const float* params32, const void* params_lp, const int64_t* text_ids,
                              const void* patches, const int32_t* co_mask, void* stash, void* workspace, const float* dxn, void* dpatches,
                              float* dtext, float* G, uint32_t drop_seed, float drop_p, const rmcl_ragged* ragged, const void* params_lpT,
                              const int32_t* replaced, int64_t mask_token_off, void* stream) {
  RMCL_REQUIRE(!replaced || (mask_token_off >= 0 && mask_token_off % 4 == 0), "encoder_backward_mpp: bad mask_token offset");
  return encoder_backward_impl(d, mode, params32, params_lp, text_ids, patches, co_mask, stash, workspace, dxn, 0, dpatches, dtext, G,
                               drop_seed, drop_p, ragged, params_lpT, replaced, mask_token_off, stream);
}

}  // extern "C"
