/* cistgcn_hip.h — C ABI of libcistgcn_hip.so, the MI355X (gfx950) kernel library behind the
 * CIST-GCN forward/backward hot path.
 *
 * The reference (QualityMinds/cistgcn) is pure Python on stock PyTorch ops: it has no FFI for this
 * path (SURVEY.md §2 "Native / kernel / collective inventory: none").  The boundary a maintainer
 * binds is therefore the set of aten-op groups inside
 *   human_motion_prediction/models/CISTGCN/CISTGCN.py   (CISTGCN.forward, :567-597)
 *   human_motion_prediction/models/layers/SE.py
 *   human_motion_prediction/losses/losses.py:50-61      (mpjpe; :36-47, :64-76, :241-267 the other training losses)
 * Each entry point below names the reference lines it replaces.  INTEGRATION.md shows the ctypes
 * binding that goes into the reference's model file.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer to fp32 data unless the type says otherwise; the caller
 *    (PyTorch in the shipped host code) owns all memory, nothing is allocated or freed here;
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing synchronises
 *    with the host, so every call is capturable into a hipGraph;
 *  - return value: 0 = ok, > 0 = hipError_t of the failed runtime call / launch,
 *    -1 = bad argument (null pointer, option without its buffer), -2 = unsupported shape;
 *  - re-entrant: no global state.
 */
#ifndef CISTGCN_HIP_H
#define CISTGCN_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* BatchNorm channel sums ("stats" / "ystats" below) are [CG_STAT_REPLICAS][C][2] f64 buffers, zero on entry:
 * every workgroup adds {sum, sum of squares} into replica (block id mod CG_STAT_REPLICAS) so that f64 atomics do
 * not serialise on one address (with thousands of workgroups per channel: tens of microseconds); the consumer sums the replicas. */
#define CG_STAT_REPLICAS 16
/* The gradient of a shared PReLU slope (one scalar per tensor) is accumulated as CG_ALPHA_SLOTS partial sums behind the channel
 * sums of a `red` buffer: same-address f64 atomics serialise at ~20 ns each on MI355X (measured, profiles/README.md), 4096 of them
 * on one word cost more than the kernel's memory traffic. */
#define CG_ALPHA_SLOTS 64

/* 4-D strided view: n[0] batch, n[1] channel, n[2] x n[3] positions; s[] in elements.
 * NCTV, NTCV (CISTGCN.py:582) and (N,3,V,T) (:592) views of one buffer differ only in s[]. */
typedef struct CgView4 {
  long long n[4];
  long long s[4];
} CgView4;

/* ---- generic strided contraction --------------------------------------------------------------
 * Y[g,m,n] = sum_k A[g,m,k] X[g,k,n] (+ bias[m]); g,m,n,k are composite indices given as int32
 * element-offset tables, concatenated in `tables` in this order:
 *   A_g[G] X_g[G] Y_g[G] | A_m[M] Y_m[M] bias_m[M] | X_n[N] Y_n[N] | A_k[K] X_k[K]
 * Replaces: nn.Conv2d 1x1 / (T,1) / (1,V) / dilated 3x3 (CISTGCN.py:54-72,138-153,165-170,229-234,
 * 305,323-340,408-418,454-458,541-545), nn.Linear (:341-352,421-440, SE.py), the adjacency
 * products torch.einsum (:122-124) and torch.matmul / bmm outer products (:187,:471), and the
 * weight / input gradients of all of them.  splitk > 1 accumulates with fp32 atomics into a dense
 * output of y_dense_numel = G*M*N elements which is zeroed here first.  `stats` (optional, f64
 * [channels][2], zero on entry, splitk == 1 only) receives per-channel sum / sum of squares of Y,
 * channel = bias_m[m]: the reduction half of the BatchNorm that follows the convolution. */
int cg_contract(const float* A, const float* X, float* Y, const float* bias, double* stats, const int32_t* tables,
                int G, int M, int N, int K, int splitk, int a_kfast, int x_kfast,
                long long y_dense_numel, void* stream);

/* Horizontal fusion: up to CG_MAX_BATCH independent contractions in ONE launch (same-depth maps of the parallel branches
 * of a DSTD_GC block - gate s/t, the four Map2Adj towers, residual maps - and, in backward, every dA / dX / bias
 * sum of such a stage).  Split-K and accumulate outputs must be zero on entry (input gradients of maps that
 * share one input are accumulated into ONE buffer instead of being summed by extra kernels). */
#define CG_MAX_BATCH 16
typedef struct CgContractDesc {
  const float* A; const float* X; float* Y; const float* bias; double* stats; const int32_t* tab;
  int G, M, N, K, splitk, kchunk /* set by the library */, a_kfast, x_kfast;
  int accumulate;                /* 1: fp32 atomic adds into a zeroed Y shared by several problems */
  int x_vec;                     /* 1: X contiguous + 16-byte aligned along n in groups of four (float4 loads) */
  int stat_ch;                   /* channels of `stats`: it holds CG_STAT_REPLICAS x stat_ch x 2 doubles */
  int mode;                      /* 0: tiled kernel.  1: streaming kernel for pointwise maps over a long position axis:
                                    requires x_vec, K <= 128, splitk 1, and Y contiguous along n in 16-byte aligned groups of
                                    four (the n offsets of Y as those of X).  2: K-reduction kernel for weight gradients (few outputs, K = batch x
                                    positions): requires K % 4 == 0, A and X contiguous along k in 16-byte aligned groups of
                                    four, no `stats`, K / splitk <= 4080, and `ws` */
  long long block0;              /* set by the library: first block id of this problem inside the launch */
  float* ws;                     /* mode 2: ZEROED scratch of cg_contract_kred_ws_floats(G, M, N) floats */
  int chain;                     /* mode 1: 1 + index (in `descs`) of another mode-1 problem with the same G, M, N whose product is
                                    added to this one's output in registers (the input gradient of a tensor that feeds several
                                    pointwise maps); the chained problem writes nothing itself (no bias / stats).  0 = none */
  int pad2;
} CgContractDesc;
int cg_contract_many(const CgContractDesc* descs, int n, void* stream);
long long cg_contract_kred_ws_floats(int G, int M, int N);

/* ---- per-channel statistics and the fused BatchNorm / Dropout / PReLU row kernel ---------------
 * stats[c] = { sum, sum of squares } over batch and positions of x*pre (f64, must be zero on entry).
 * Replaces the reduction half of nn.BatchNorm{1,2}d in train mode. */
int cg_chan_stats(const float* x, const CgView4* xv, const float* pre, double* stats, void* stream);
#define CG_ROW_MAX_BATCH 6       /* problems per launch of the row kernels (cg_chan_stats_many, cg_norm_act_*_many): kernel-argument budget */
typedef struct CgStatsArgs { const float* x; CgView4 xv; const float* pre; double* stats; } CgStatsArgs;
int cg_chan_stats_many(const CgStatsArgs* items, int n, void* stream);   /* up to CG_ROW_MAX_BATCH tensors per launch */
/* out[c] += sum over batch and positions (bias gradients of the convolutions); `out` (C floats) zero on entry. */
int cg_chan_sum(const float* x, const CgView4* xv, float* out, void* stream);

/* y = PReLU( Dropout( (x*pre)*scale + shift ) [+ add] ) [+ add if add_post]
 * with (scale, shift) from batch statistics (bn_mode 1, also updates running stats exactly like
 * nn.BatchNorm: momentum, unbiased running_var), running statistics (bn_mode 2) or identity (0).
 * Replaces every Conv->BN->[Dropout]->[PReLU] tail, `tcn + residual -> PReLU` (CISTGCN.py:266-269),
 * `PReLU(BN(w*x))` (:388), the SE channel scale (SE.py:20,41) and the residual sums (:390,:586). */
typedef struct CgNormAct {
  const float* x;  CgView4 xv;
  float* y;        CgView4 yv;
  const float* pre;              /* (B,C) per-sample channel gate or NULL */
  const float* add; CgView4 av;  /* addend (same logical shape) or NULL */
  int add_post;                  /* 0: before the PReLU, 1: after it */
  int bn_mode;                   /* 0 none, 1 batch statistics, 2 running statistics */
  const double* stats;           /* [C][2], bn_mode 1 */
  const float* gamma; const float* beta;
  float* running_mean; float* running_var; long long* num_batches_tracked;
  float momentum, eps;
  float* save_mean; float* save_rstd;   /* [C] written by fwd, read by bwd */
  float drop_p; const unsigned long long* seed; unsigned int salt;
  const float* alpha; int alpha_n;      /* PReLU slope(s) (1 or C) or NULL */
  /* backward only */
  const float* dy; CgView4 dyv;
  float* dx; CgView4 dxv;
  float* dadd; CgView4 dav;      /* gradient of a pre-activation addend (NULL: not needed) */
  float* dpre;                   /* (B,C) or NULL */
  double* red;                   /* [2C + (alpha_n == 1 ? CG_ALPHA_SLOTS : alpha_n)] f64 scratch, zero on entry: per channel sum g, sum g * xhat,
                                    the slope sums behind them */
  float* dgamma; float* dbeta; float* dalpha;
  double* ystats;                /* forward, optional: [C][2] f64 sums of y (zero on entry) for the BatchNorm consuming y */
} CgNormAct;
int cg_norm_act_fwd(const CgNormAct* a, void* stream);
int cg_norm_act_bwd(const CgNormAct* a, int need_reduce, void* stream);
/* the same for up to CG_ROW_MAX_BATCH independent row problems per launch (branches of one block at the same depth) */
int cg_norm_act_fwd_many(const CgNormAct* arr, int n, void* stream);
int cg_norm_act_bwd_many(const CgNormAct* arr, const int* need_reduce, int n, void* stream);
/* pass 1 of the backward alone (channel sums, slope gradient) + dgamma / dbeta / dalpha: for a consumer that applies the BatchNorm / PReLU
 * backward itself while loading the gradient (cg_pointwise_maps_bwd with yraw) */
int cg_norm_act_bwd_reduce_many(const CgNormAct* arr, int n, void* stream);

/* per-(b,c) mean (kind 0), max with first arg-max (kind 1) or sum (kind 2) over the positions; adjoints of 0/1.
 * Replaces AdaptiveAvgPool (SE.py:8,27; CISTGCN.py:69,76), .max(-1)[0] chains and .mean((2,3))
 * (CISTGCN.py:465-467). */
int cg_reduce_bc(const float* x, const CgView4* xv, int kind, float* out, int32_t* arg, void* stream);
int cg_reduce_bc_bwd(const float* dout, const int32_t* arg, int kind, float* dx, const CgView4* dxv, void* stream);

/* y = a (+ b) (+ c) on strided views: torch.cat slices (CISTGCN.py:77,378-380,388,468), halo
 * padding for the dilated FPN convolutions (:54-68), F.interpolate broadcast (:76), the tail
 * x[:, -1:] + x8^T + act (:595-597). */
/* y = a[0] + ... + a[n-1] (n <= CG_SUM_MAX), same logical shape, any strides: sums the gradients of a multi-consumer tensor in one
 * launch (replaces autograd's one accumulation kernel per extra consumer) */
#define CG_SUM_MAX 8
typedef struct CgSumItem { const float* a; CgView4 av; } CgSumItem;
int cg_sum_many(float* y, const CgView4* yv, const CgSumItem* items, int n, void* stream);
int cg_add3(float* y, const CgView4* yv, const float* a, const CgView4* av, const float* b, const CgView4* bv,
            const float* c, const CgView4* cv, void* stream);
#define CG_COPY_MAX 4
typedef struct CgCopyItem { float* y; CgView4 yv; const float* a; CgView4 av; } CgCopyItem;
int cg_copy_many(const CgCopyItem* items, int n, void* stream);   /* up to CG_COPY_MAX strided copies (cat slices) per launch */
int cg_zero(void* p, long long bytes, void* stream);

/* ---- stage kernels --------------------------------------------------------------------------------
 * feature lift, CISTGCN.py:568-577: x (B,T,V,3) -> (B,10,T,V) = [x, acc, vel, |vel|] and its adjoint */
int cg_feature_lift_fwd(const float* x, float* f, long long B, long long T, long long V, void* stream);
int cg_feature_lift_bwd(const float* x, const float* df, float* dx, long long B, long long T, long long V, void* stream);
/* DSTD_GC._get_stats_, CISTGCN.py:360-371: contiguous (B,C,T,V) -> (B, 2+2T) */
int cg_dstd_stats_fwd(const float* x, float* out, int B, int C, int T, int V, void* stream);
int cg_dstd_stats_bwd(const float* x, const float* dout, float* dx, int B, int C, int T, int V, void* stream);
/* SELayer excitation, SE.py:9-14,30-35: gate = sigmoid(W2 relu(W1 pooled)); W1 (H,C), W2 (C,H) */
int cg_se_gate_fwd(const float* pooled, const float* W1, const float* W2, float* gate, int B, int C, int H, void* stream);
int cg_se_gate_bwd(const float* pooled, const float* W1, const float* W2, const float* gate, const float* dgate,
                   float* dpooled, float* dW1, float* dW2, int B, int C, int H, int prezeroed, void* stream);
/* prezeroed != 0: dW1/dW2 are already zero (slices of the per-step zero pool), no memset is issued */
/* rank-1 adjacency seed of Map2Adj, CISTGCN.py:183-189 (`torch.matmul` of the joint and time summaries): s (B,V,T) and
 * q (B,T,V) contiguous; domain 0: o[b,v,t,u] = s[b,v,t]*q[b,u,v] (B,V,T,T); domain 1: o[b,t,v,w] = s[b,v,t]*q[b,t,w]
 * (B,T,V,V).  Up to two problems (the space and time tower of one block) per launch; backward reads d o once and writes
 * both d s and d q.  T, V <= 64; o / dout 16-byte aligned. */
typedef struct CgRank1 { const float* s; const float* q; float* o; const float* dout; float* ds; float* dq; int domain; int pad; } CgRank1;
int cg_rank1_adj_fwd(const CgRank1* items, int n, int B, int T, int V, void* stream);
int cg_rank1_adj_bwd(const CgRank1* items, int n, int B, int T, int V, void* stream);
/* cumsum over axis 1 of a strided 4-D view (B,L,R1,R2), CISTGCN.py:589 (reverse = adjoint) */
int cg_cumsum(const float* x, const CgView4* xv, float* y, const CgView4* yv, int reverse, void* stream);
/* MPJPE, losses/losses.py:50-61 (reduce_axis=[]): pred/target contiguous (N,3); loss is one float */
int cg_mpjpe_fwd(const float* pred, const float* tgt, float* loss, long long N, void* stream);
int cg_mpjpe_bwd(const float* pred, const float* tgt, const float* gloss, float* dpred, long long N, void* stream);
/* advances the device-resident dropout seed (one word) once per training step */
int cg_seed_bump(unsigned long long* seed, void* stream);

/* ---- fused ST-GCN stage (the dominant kernel) ---------------------------------------------------
 * Domain_GCNN_layer core, CISTGCN.py:265-266 with :122-124:
 *   y[b,co,.,.] = bias[co] + sum_ci W[co,ci] * G[b,ci,.,.],
 *   G = einsum('nctv,nvtq->ncqv', x, Adj)  (domain 0, Adj (B,V,T,T))   or
 *       einsum('nctv,ntvw->nctw', x, Adj)  (domain 1, Adj (B,T,V,V)).
 * x, y contiguous (B,C,T,V).  Adjacency is staged in LDS, the graph product and the channel mix
 * run back to back without the intermediate G touching HBM.  Optional per-channel f64 sums of y
 * (ystats, [Cout][2], zero on entry) feed the train-mode BatchNorm that follows (:235).
 * Backward: dx, dAdj, dW, db from dy.  dW/db partial sums go through `ws`, a caller-owned scratch of
 * cg_stgcn_domain_bwd_ws_floats(Cin, Cout) floats (zeroed here unless ws_prezeroed != 0; replicated accumulators
 * keep the fp32 atomics off a single address), and are folded into dW/db by a second tiny kernel.
 * Wide layers (16+ channels) at batch sizes that fill the chip run as plane kernels (csrc/stgcn_domain_planes.hip: the channel
 * mix first, on whole plane rows; LDS transposes to the group-major order of the graph product); smaller launches use the tile
 * kernels.  cg_stgcn_domain_planes_min_workgroups(n) moves that switch (n workgroups; returns the previous value, n < 0 only
 * reads it): both generations compute the same function, tests pin either one. */
long long cg_stgcn_domain_planes_min_workgroups(long long n);
int cg_stgcn_domain_fwd(const float* x, const float* adj, const float* W, const float* bias, float* y, double* ystats,
                        int B, int Cin, int Cout, int T, int V, int domain, void* stream);
long long cg_stgcn_domain_bwd_ws_floats(int Cin, int Cout);
int cg_stgcn_domain_bwd(const float* x, const float* adj, const float* W, const float* dy, float* dx, float* dadj,
                        float* dW, float* dbias, float* ws, int B, int Cin, int Cout, int T, int V, int domain,
                        int ws_prezeroed, void* stream);

/* ---- tail of a DSTD_GC block as phase kernels (SURVEY 8b `dstd_combine`) ------------------------------------------------
 * CISTGCN.py:266-269 (`tcn` BatchNorm + Dropout + residual + PReLU of both Domain_GCNN layers), :388 (PReLU(BN(w * x)) of both
 * branches + cat), :305-309 (compressor 1x1 conv + BN + PReLU + SELayer2d), :390 (block residual).  In train mode every
 * BatchNorm needs the batch statistics of its input first, so the chain is cut at those barriers and nowhere else:
 *   forward  phase 1: sums of z_i = w_i * PReLU(Dropout(BN(y_i)) + r_i) | 2: h0 = Wc [a_1; a_2] on the matrix cores, a_i =
 *            PReLU(BN(z_i)) rebuilt per tile, + sums of h0 | 3: pooled = mean PReLU(BN(h0)) | (cg_se_gate_fwd) | 4: out = h * gate
 *            + block residual (+ sums of out for the next block's BatchNorm);
 *   backward phase 1: dgate | (cg_se_gate_bwd) | 2: sums at the compressor BatchNorm | 3: dh0, d a = Wc^T dh0, dWc on the matrix
 *            cores, gradient in front of prelu1/2 + its sums | 4: gate gradients dw, gradient of the residual addends, sums of
 *            the tcn BatchNorm | 5: dy_i and every per-channel parameter gradient (with `red_q`: 4 does both passes, 6 the parameters).
 * All tensors contiguous (B,C,T,V) / (B,C); C <= 64.  `stats` / `red_*` / `dWc_ws` are zeroed by the caller (slices of the
 * per-step arenas); BatchNorm bookkeeping (save mean / rstd, running statistics) as cg_norm_act. */
typedef struct CgTailBN {
  double* stats;                 /* [CG_STAT_REPLICAS][C][2] {sum, sum of squares} of this BatchNorm's INPUT over batch and positions (train mode
                                    only; zero before the producing phase) */
  const float* gamma; const float* beta;
  float* running_mean; float* running_var; long long* num_batches_tracked;
  float momentum, eps;
  float* save;                   /* [2][C] mean, rstd used by the forward (written by the first phase that needs them, read by the later phases
                                    and the backward) */
} CgTailBN;
typedef struct CgDstdTail {
  int B, C, T, V, train, pad0;
  const float* y[2];             /* tcn outputs of the space / time Domain_GCNN layer (B,C,T,V), pre-BatchNorm */
  const float* r[2];             /* their residual addends (B,C,T,V): the block input or the residual conv + BN */
  const float* w[2];             /* gates w1 / w2 (B,C) */
  CgTailBN bn_t[2]; const float* alpha_d[2];      /* tcn.1 + layer PReLU */
  CgTailBN bn_p[2]; const float* alpha_p[2];      /* prelu1 / prelu2 (BatchNorm + PReLU) */
  const float* Wc; CgTailBN bn_c; const float* alpha_c;   /* compressor conv (C, 2C), BN, PReLU */
  const float* gate; const float* bres;           /* SE gate (B,C), block residual (B,C,T,V) */
  float drop_p; unsigned int salt[2]; int pad1; const unsigned long long* seed;
  float* h0; float* pooled; float* out; double* ostats;      /* forward results (ostats optional: sums of out) */
  float* tap_x[2]; float* tap_a[2]; float* tap_h;      /* optional taps (B,C,T,V): outputs of the layer PReLUs, of prelu1/2, of the compressor
                                                          PReLU - not needed by the computation (diagnostics / branch records) */
  /* backward */
  const float* dout; const float* dpooled; float* dgate;
  double* red_c;                 /* [2C + CG_ALPHA_SLOTS] f64, zero on entry: channel sums, then the spread partial sums of d alpha */
  float* gp[2]; double* red_p[2];    /* gradient in front of prelu1/2's BatchNorm (B,C,T,V); [2C + CG_ALPHA_SLOTS] f64 each, zero on entry */
  float* dWc_ws; float* dWc;     /* cg_dstd_tail_ws_floats(C) zeroed scratch; (C, 2C) */
  float* dr[2]; float* dw[2]; double* red_t[2]; float* dy[2];
  float* dgamma_t[2]; float* dbeta_t[2]; float* dalpha_d[2];
  float* dgamma_p[2]; float* dbeta_p[2]; float* dalpha_p[2];
  float* dgamma_c; float* dbeta_c; float* dalpha_c;
  double* rows_c;                /* optional, backward phases 1 and 2 together: [B][C][6] f64 scratch (nothing to zero).  Phase 1 leaves six row
                                  * sums per (b, c) in it and phase 2 forms red_c from them and gate / dpooled with plain stores in a fixed
                                  * order - no pass over dout and h0, red_c need not be zero, the same bits from run to run */
  /* optional: the tcn BatchNorm's backward sums a phase early.  With `red_q` and T * V % 4 == 0 backward phase 4 writes dy as well and phase
   * 5 is replaced by phase 6 (the per-channel parameter gradients, one small launch); train mode then needs `fmom` from forward phase 1. */
  double* fmom[2];               /* [CG_STAT_REPLICAS][C][4] f64, zero before forward phase 1 (train): moments of q = keep PReLU_d'(u) w
                                    (sums of q, q z, q yhat, q z yhat) */
  double* red_q[2];              /* [CG_STAT_REPLICAS][C][2] f64, zero before backward phase 3: sums of q g_p, q g_p (y - mean_t) */
  int rs_shared, pad2;           /* with the above and r[0] == r[1] (else -1): phase 4 writes dr[0] = the sum of both residual gradients, dr[1] untouched */
} CgDstdTail;
int cg_dstd_tail_fwd(const CgDstdTail* t, int phase, void* stream);
int cg_dstd_tail_bwd(const CgDstdTail* t, int phase, void* stream);
long long cg_dstd_tail_ws_floats(int C);

/* ---- frame-collapsing convolution nn.Conv2d(C, O, (T, 1)) (no bias): first convolution of the gate paths CISTGCN.py:331-336 and
 * second convolution of Map2Adj.time_compress :138-150.  y[b,o,v] = sum_{c,t} W[o,c,t] x[b,c,t,v]; x (B,C,T,V) contiguous, W (O, C*T),
 * y (B,O,V); V <= 32, O <= 64, C*T % 4 == 0 (else CG_ESHAPE: cg_contract_many).  Forward: one workgroup per sample; backward:
 * dx and dW from one pass (workgroup = 64 rows of W x a slice of the samples). */
typedef struct CgRowsConv {
  int B, C, T, V, O, pad;
  const float* x; const float* W;
  float* y; double* stats;          /* stats: optional [CG_STAT_REPLICAS][O][2] f64 sums of y, zero on entry */
  const float* dy; float* dx; float* dW;
  float* ws;                        /* cg_collapse_rows_ws_floats(C, T, O) floats of scratch (need not be zeroed) */
  /* optional transform of the input on load (in_on != 0): x' = PReLU(BatchNorm2d(x)) over the C input channels with the shared slope
   * in_alpha[0]: the first level of a Map2Adj tower (CISTGCN.py:138-141 / :156-158) folded into the load path of its collapsing
   * convolution - the activated tensor is never stored.  Forward: in_bn.stats = f64 channel sums of x (train; workgroup 0 writes
   * in_bn.save and the running statistics), eval: running statistics.  Backward: in_bn.save; dx is then the gradient with respect to
   * x' (the BatchNorm / PReLU backward is applied by the producer of x: cg_pointwise_maps_bwd with `yraw`). */
  int in_on, in_train;
  CgTailBN in_bn;
  const float* in_alpha;
  float* in_tap;                    /* forward, optional (with in_on): the activated input x' (B,C,T,V), written as it is formed (branch records of the parity tests) */
  /* backward, optional (with in_on; `sums` and `red` together): the channel sums of the BatchNorm / PReLU backward of the producer of x,
   * formed from the operands the kernel holds anyway.  With gh = dx PReLU'(u) and xhat = (x - mean) rstd:
   *   red[2c] = sum gh, red[2c + 1] = sum gh xhat, red[2C] = sum_{u <= 0} dx u, red[2C + 1 .. 2C + CG_ALPHA_SLOTS - 1] = 0
   * - what cg_norm_act_bwd_reduce_many leaves for cg_pointwise_maps_bwd (`bn_red`), summed in a fixed order (nothing to zero, the same
   * bits from run to run); dgamma[c] = red[2c + 1], dbeta[c] = red[2c], dalpha[0] = red[2C] (each optional). */
  double* sums;                     /* cg_collapse_sums_ws_floats(C, T) (rows) / (C, V) (cols) floats of scratch (need not be zeroed) */
  double* red;                      /* [2C + CG_ALPHA_SLOTS] f64 */
  float* dgamma; float* dbeta; float* dalpha;
} CgRowsConv;
int cg_collapse_rows_fwd(const CgRowsConv* t, void* stream);
int cg_collapse_rows_bwd(const CgRowsConv* t, void* stream);
long long cg_collapse_rows_ws_floats(int C, int T, int O);
/* The same for the joint axis: nn.Conv2d(C, O, (1, V)) (no bias), second convolution of Map2Adj.joint_compress, CISTGCN.py:152-163.
 * y[b,o,t] = sum_{c,v} W[o,c,v] x[b,c,t,v]; same argument block with W (O, C*V), y (B,O,T), dy (B,O,T), ws of
 * cg_collapse_cols_ws_floats(C, V, O) floats of scratch; T <= 64, O <= 64, C*V % 4 == 0 (cg_collapse_cols_supported; else cg_contract_many). */
int cg_collapse_cols_fwd(const CgRowsConv* t, void* stream);
int cg_collapse_cols_bwd(const CgRowsConv* t, void* stream);
int cg_collapse_cols_supported(int C, int T, int V, int O);
long long cg_collapse_cols_ws_floats(int C, int V, int O);
/* host-only: floats of CgRowsConv.sums for C channels of `rows` rows each (rows = T for cg_collapse_rows_bwd, V for cg_collapse_cols_bwd), any B */
long long cg_collapse_sums_ws_floats(int C, int rows);

/* ---- dilated 3x3 convolutions of the time extrapolator, FPN CISTGCN.py:54-79: n <= 3 convolutions with padding = dilation =
 * dil[i] of ONE input (B,C,H,W) = (batch, frames, channels, joints).  A sample fits in LDS with its halo: forward, input gradient
 * (summed over the convolutions) and weight / bias gradients each walk whole samples.  H * W % 4 == 0, H * W <= 256, C <= 64, O <= 32 and the
 * sample's halo image plus one weight matrix must fit in LDS; shapes outside cg_fpn_conv_supported: CG_ESHAPE (the caller uses cg_contract_many). */
typedef struct CgFpnConv {
  int B, C, O, H, W, n;
  int dil[3]; int pad;
  const float* x; long long xs[3];     /* element strides of x: batch, channel, row; unit stride along W */
  const float* w[3]; const float* bias[3];      /* (O,C,3,3); bias may be NULL */
  float* y[3];                   /* (B,O,H,W) contiguous */
  /* backward */
  const float* dy[3];
  float* dx;                     /* optional: sum over the convolutions */
  float* dw[3]; float* db[3];    /* optional each */
  float* ws;                     /* cg_fpn_conv_ws_floats(B, C, O, n) floats of scratch */
} CgFpnConv;
int cg_fpn_conv_fwd(const CgFpnConv* t, void* stream);
int cg_fpn_conv_bwd(const CgFpnConv* t, void* stream);
int cg_fpn_conv_supported(int B, int C, int O, int H, int W);
long long cg_fpn_conv_ws_floats(int B, int C, int O, int n);

/* ---- stacked pointwise maps of one input: the first convolutions of the Map2Adj towers of a block, CISTGCN.py:138-163 applied
 * to the normalised block input by :183-186 (up to four 1x1 convolutions of the same (B,C,T,V) tensor).  Forward: every y_i =
 * W_i x from one read of x, with the f64 channel sums of y_i (train-mode BatchNorm behind it).  Backward: dx = sum_i W_i^T dy_i and
 * every dW_i = dy_i x^T from one read of x and of each dy_i.  x (B,Cin,P) contiguous, P = T*V with P % 2 == 0 (rows of 16- or 8-byte alignment), Cin <= CG_PWM_MAXCIN,
 * M_i <= CG_PWM_MAXM, sum of ceil16(M_i) <= CG_PWM_MAXROWS, (sum of ceil16(M_i) / 16) * ceil(Cin / 16) <= 32; other shapes: CG_ESHAPE (the caller
 * uses cg_contract_many). */
#define CG_PWM_MAXN 4        /* maps per launch */
#define CG_PWM_MAXROWS 128   /* sum of the maps' output channels, each rounded up to 16 */
#define CG_PWM_MAXCIN 128    /* input channels */
#define CG_PWM_MAXM 64       /* output channels of one map */
typedef struct CgPwMaps {
  int B, Cin, P, n;
  const float* x;
  const float* W[CG_PWM_MAXN]; int M[CG_PWM_MAXN];       /* (M_i, Cin) */
  float* y[CG_PWM_MAXN];                                 /* (B, M_i, P) */
  double* stats[CG_PWM_MAXN];                            /* all null, or [CG_STAT_REPLICAS][M_i][2] each, zero on entry */
  /* backward */
  const float* dy[CG_PWM_MAXN];
  float* dx;                                             /* (B, Cin, P): sum over the maps of W_i^T dy_i */
  float* dW[CG_PWM_MAXN];                                /* (M_i, Cin) */
  float* dW_ws;                                          /* cg_pointwise_maps_ws_floats(Cin) zeroed floats (replicated accumulators) */
  const float* bias[CG_PWM_MAXN];                        /* optional (M_i): y_i = W_i x + bias_i (nn.Conv2d(..., 1) with bias: the residual maps) */
  float* db[CG_PWM_MAXN];                                /* backward, optional (M_i): bias gradient, sum of dy_i over batch and positions */
  /* backward, optional (all maps or none): BatchNorm2d + PReLU follow the maps (the Map2Adj towers, CISTGCN.py:138-141) and dy_i is the
   * gradient BEHIND them; the kernel undoes both while it loads dy_i (raw outputs yraw, saved mean / rstd [2][M_i], gamma, beta, the sums
   * `bn_red` [M_i][2] f64 of cg_norm_act_bwd_reduce_many, the slope) */
  const float* yraw[CG_PWM_MAXN];
  const float* bn_save[CG_PWM_MAXN]; const float* bn_gamma[CG_PWM_MAXN]; const float* bn_beta[CG_PWM_MAXN];
  const double* bn_red[CG_PWM_MAXN]; const float* prelu[CG_PWM_MAXN];
  int bn_train, pad;                                     /* 1: batch statistics (the sums enter dy), 0: running statistics */
} CgPwMaps;
int cg_pointwise_maps_fwd(const CgPwMaps* t, void* stream);
int cg_pointwise_maps_bwd(const CgPwMaps* t, void* stream);
long long cg_pointwise_maps_ws_floats(int Cin);

/* ---- tail of the interpretability map, Map2Adj.forward CISTGCN.py:183-189 (expansor :165-170) ------------------------
 * s (B,V,T), q (B,T,V): outputs of the joint / time towers.  Seed o = s (x) q (space: o[b,v,t,u] = s[b,v,t] q[b,u,v];
 * time: o[b,t,v,w] = s[b,v,t] q[b,t,w]) -> conv W0 over the slab axis -> BatchNorm -> Dropout -> PReLU -> conv W4 = Adj.
 * The seed is generated inside the kernels, never stored.  `items`: the towers of a block sharing a launch (n <= 2, same B).
 *   forward phase 1: e = W0 o + f64 channel sums | 2: Adj = W4 PReLU(Dropout(BN(e)))
 *   backward phase 1: g = gradient in front of the BatchNorm, its sums, d alpha, dW4 | 2: d e, ds, dq, dW0, d gamma / d beta
 * domain 0 (space): Kc = V, J = T; domain 1 (time): Kc = T, J = V; Kc, J <= 64.  `bn.stats`, `red`, `dW*_ws` zeroed by the caller. */
typedef struct CgAdjTail {
  int B, Kc, J, domain, train, pad0;
  const float* s; const float* q;
  const float* W0; CgTailBN bn; const float* alpha; const float* W4;
  float drop_p; unsigned int salt; const unsigned long long* seed;
  float* e; float* adj;          /* (B,Kc,J,J): first conv output (kept for the backward), the adjacency */
  float* tap;                    /* optional (B,Kc,J,J): PReLU output (diagnostics / branch records) */
  /* backward */
  const float* dadj; float* g; double* red;       /* g (B,Kc,J,J) scratch; red: cg_map2adj_tail_red_doubles(Kc) f64 words */
  float* ds; float* dq; float* part;   /* part: cg_map2adj_tail_part_floats(B, Kc, J) floats of scratch */
  float* dW0_ws; float* dW4_ws;  /* cg_map2adj_tail_ws_floats(Kc) / 2 floats each */
  float* dW0; float* dW4; float* dgamma; float* dbeta; float* dalpha;
} CgAdjTail;
int cg_map2adj_tail_fwd(const CgAdjTail* items, int n, int phase, void* stream);
int cg_map2adj_tail_bwd(const CgAdjTail* items, int n, int phase, void* stream);
long long cg_map2adj_tail_ws_floats(int Kc);
long long cg_map2adj_tail_part_floats(int B, int Kc, int J);
long long cg_map2adj_tail_red_doubles(int Kc);

/* ---- head of a DSTD_GC block, DSTD_GC.forward CISTGCN.py:375-379 with _get_stats_ :360-371 ---------------
 * xn = global_norm(x) (BatchNorm2d) and the block statistics of xn from one pass over x; backward: the gradients of all consumers of
 * xn (g[0..ng-1], null entries skipped), the gradient of the statistics (dout[0] + dout[1]) and the BatchNorm backward in two
 * streaming passes.  x (B,C,T,V) contiguous with T*V <= 4608 (cg_block_input_supported; else CG_ESHAPE: cg_norm_act + cg_dstd_stats).
 * Forward (two launches) writes xn, rm / rq ((B,C,T) row means and centred sums of squares, read again by the backward), out
 * (B, 2+2T) and bn.save; train mode needs bn.stats = f64 sums of x.  Backward (three launches) needs pq (B,C,T,2) and gsum (B,C,T,V)
 * scratch and red = [CG_STAT_REPLICAS][C][2] zeroed f64 words; writes dx, dgamma, dbeta. */
#define CG_BIN_MAXG 8
typedef struct CgBlockInput {
  int B, C, T, V, train, ng;
  const float* x;               /* (B,C,T,V) contiguous block input */
  CgTailBN bn;                  /* global_norm; bn.stats: [CG_STAT_REPLICAS][C][2] f64 sums of x (train); bn.save [2][C] mean / rstd */
  float* xn;                    /* (B,C,T,V) normalised input */
  float* rm; float* rq;         /* (B,C,T) mean / centred sum of squares of every row of V joints of xn (kept for the backward) */
  float* out;                   /* (B, 2 + 2T) block statistics of xn */
  /* backward */
  const float* g[CG_BIN_MAXG];  /* gradients with respect to xn from its consumers, (B,C,T,V) contiguous, ng of them (null entries skipped) */
  const float* dout[2];         /* gradients of `out` from its (up to two) consumers, (B, 2 + 2T); null entries skipped */
  long long dout_ld[2];         /* their row strides in floats (column slices of a wider tensor are taken as they are) */
  float* pq;                    /* (B,C,T,2) scratch: slope / offset of the statistics' gradient per row, d xn += (xn - rm) P + Q */
  float* gsum;                  /* (B,C,T,V) scratch: the summed gradient in front of the BatchNorm (eval mode: may alias dx) */
  double* red;                  /* [CG_STAT_REPLICAS][C][2] f64, zero on entry */
  float* dx; float* dgamma; float* dbeta;
} CgBlockInput;
int cg_block_input_fwd(const CgBlockInput* t, void* stream);
int cg_block_input_bwd(const CgBlockInput* t, void* stream);
int cg_block_input_supported(int B, int C, int T, int V);

/* ---- tail of the gate paths of a DSTD_GC block, conv_s / conv_t slots 5-7 and map_s / map_t, CISTGCN.py:337-352 / :378-384 ------
 * per path: z (B,C) -> BatchNorm2d -> Dropout -> PReLU -> cat with the block statistics (B,S) -> Linear (C, C+S) -> BatchNorm1d -> Dropout ->
 * PReLU -> Linear (C,C) = the gate (B,C).  A workgroup owns sixteen samples;
 * two launches forward, three backward, for both paths (cut only at the batch statistics, which every workgroup computes itself).  C <= CG_GATE_MAXC,
 * S <= CG_GATE_MAXS (cg_gate_head_supported; else CG_ESHAPE: cg_norm_act_* +
 * cg_copy_many + cg_contract_many).  Forward writes y (B,C: the first Linear's output, kept for the backward), w, both bn.save;
 * backward needs `scratch` = cg_gate_head_scratch_floats(B, C, S) floats and `red` = two zeroed f64 words per path, dWl / dW2 ZERO on entry
 * (accumulated with float atomics), and writes dz, dstats (B,S) and every parameter gradient. */
#define CG_GATE_MAXC 64
#define CG_GATE_MAXS 192
typedef struct CgGatePath {
  const float* z;               /* (B,C) contiguous: output of the joint-collapsing convolution conv_p[4] */
  const float* stats; long long stats_ld;      /* (B,S) block statistics, S = 2 + 2T; row stride in floats */
  CgTailBN bn2; const float* alpha2;           /* bn.stats unused (the kernel reduces over the batch itself); bn.save [2][C] */
  const float* Wl;              /* (C, C+S) */
  CgTailBN bn3; const float* alpha3;
  const float* W2;              /* (C, C) */
  unsigned int salt2, salt3;    /* dropout site ids of the two Dropout layers */
  float* y;                     /* (B,C) Linear output in front of bn3 (kept for the backward) */
  float* w;                     /* (B,C) result */
  float* tap2; float* tap3;     /* optional (B,C): the two PReLU outputs (diagnostics / branch records) */
  /* backward */
  const float* dw;              /* (B,C) */
  float* dz;                    /* (B,C) */
  float* dstats;                /* (B,S) contiguous */
  float* dWl; float* dW2;
  float* dgamma2; float* dbeta2; float* dalpha2; float* dgamma3; float* dbeta3; float* dalpha3;
  float* scratch;               /* cg_gate_head_scratch_floats(B, C, S) floats (the gradients in front of the two BatchNorms) */
  double* red;                  /* two f64 words, zero on entry (slope sums) */
} CgGatePath;
typedef struct CgGateHead {
  int B, C, S, train, n, pad;   /* n paths (1 or 2) */
  float drop_p; int pad2; const unsigned long long* seed;
  CgGatePath p[2];
} CgGateHead;
int cg_gate_head_fwd(const CgGateHead* t, void* stream);
int cg_gate_head_bwd(const CgGateHead* t, void* stream);
int cg_gate_head_supported(int B, int C, int S);
long long cg_gate_head_scratch_floats(int B, int C, int S);

/* ---- middle of a DSTD_GC block (csrc/block_mid.hip): CISTGCN.py:331-352 (conv_s|t slots 5-7 and the (1,V) convolution) and :138-163
 * (time_compress / joint_compress slots 4-6) --------------------------------------------------------------------------
 * up to CG_MID_MAXN items, each x (B,C,L) -> BatchNorm2d -> Dropout [-> PReLU] = h, then
 *   kind 0 (full):      y[b,o]   = sum_{c,l} W[o,c,l] h[b,c,l]     (B,O)
 *   kind 1 (pointwise): y[b,o,l] = sum_c W[o,c] h[b,c,l]           (B,O,L)
 * C, L, O <= 64.  One launch forward (train mode: bn.stats = the producer's replicated f64 sums of x, rows of stats_ld channels), two backward,
 * cut at the batch statistics.  Backward scratch per item (sizes from cg_block_mid_geometry, nothing has to be zero): g (B,C,L) floats, `part`
 * doubles, `wpart` floats.  No atomics: every gradient is the same from run to run.  sb_ / ns_ are filled in by the launcher. */
#define CG_MID_MAXN 6
typedef struct CgMidItem {
  int kind, C, L, O;
  int sb_, ns_;                 /* samples per slice, slices: filled in by the launcher (cg_block_mid_geometry) */
  const float* x; long long x_ld;      /* (B,C,L), sample stride in floats (rows of C*L floats are dense) */
  CgTailBN bn; long long stats_ld;     /* bn.stats: [CG_STAT_REPLICAS][stats_ld][2] f64 sums of x, this item's channels from c = 0 (train) */
  const float* alpha;           /* optional single PReLU slope */
  const float* W;               /* (O, C*L) | (O, C) */
  unsigned int salt; int pad;
  float* y;                     /* (B,O) | (B,O,L) */
  float* tap;                   /* optional (B,C,L): h (branch records) */
  /* backward */
  const float* dy;              /* like y */
  float* dx;                    /* (B,C,L) dense */
  float* dW; float* dgamma; float* dbeta; float* dalpha;
  float* g;                     /* (B,C,L) scratch: the gradient in front of the BatchNorm */
  double* part;                 /* [ns][2C+1] scratch, all written by launch 1 (see cg_block_mid_geometry) */
  float* wpart;                 /* [ns][O*C*L | O*C] scratch, all written by launch 1 */
} CgMidItem;
typedef struct CgBlockMid {
  int B, train, n, pad;
  float drop_p; int pad2; const unsigned long long* seed;
  CgMidItem it[CG_MID_MAXN];
} CgBlockMid;
int cg_block_mid_fwd(const CgBlockMid* t, void* stream);
int cg_block_mid_bwd(const CgBlockMid* t, void* stream);
int cg_block_mid_supported(int B, int kind, int C, int L, int O);
/* out[8]: samples per slice, slices, dynamic LDS bytes forward / backward, `part` doubles, `wpart` floats, passes of the full product over
 * the groups of four output rows, passes of the full backward over the columns */
int cg_block_mid_geometry(int B, int kind, int C, int L, int O, int* out);

/* ---- ContextLayer heads 1 and 3, CISTGCN.py:408-418 with :465 / :467 ---------------------------------
 * Conv2d(1, C, 1, bias=False) -> BatchNorm2d(C) -> PReLU of the one-channel tensor x (B,1,T_out,3V), reduced over the positions:
 *   head 0 (context_conv1): y[0][b,c] = max_p z (first arg-max in `arg`), head 1 (context_conv3): y[1][b,c] = mean_p z.
 * The (B,C,P) activations are functions of x[b,p] and per-channel constants (batch statistics of w[c] x are w[c] mean(x),
 * w[c]^2 var(x)); they are never stored.  x (B,P) contiguous, C <= CG_CTX_MAXC, P <= 16384 (else CG_ESHAPE: the caller composes the heads
 * from cg_pointwise_maps / cg_norm_act / cg_reduce_bc).  Train mode needs `xstats` = [CG_STAT_REPLICAS][1][2] f64 sums of x
 * (cg_chan_stats_many on the (B,1,P) view).  bn[h].save ([2][C]) and xsave ([2]) are written by the forward, read by the backward.
 * Backward: two launches (per-channel sums, then dx and the parameter gradients in closed form); `red`:
 * cg_context_heads_red_doubles(C) f64 words, zero on entry. */
#define CG_CTX_MAXC 64
typedef struct CgCtxHeads {
  int B, P, C, train;
  const float* x;
  const double* xstats;         /* train: [CG_STAT_REPLICAS][1][2] f64 {sum x, sum x^2} over batch and positions (cg_chan_stats_many) */
  const float* w[2]; CgTailBN bn[2]; const float* alpha[2];      /* bn.save: [2][C] mean / rstd of the channel (written by the forward) */
  float* y[2];                  /* (B,C) */
  int32_t* arg;                 /* (B,C) first arg-max position of head 0 */
  float* xsave;                 /* [2] mean and (biased) variance of x the forward used (train) */
  float* tap[2];                /* optional (B,C,P): the PReLU outputs (diagnostics / branch records) */
  /* backward */
  const float* dy[2];           /* (B,C) */
  double* red;                  /* [CG_STAT_REPLICAS][2][C][3] f64, zero on entry: sum gu, sum gu * x, sum over the negative side of g * u */
  float* dx;                    /* (B,P) */
  float* dw[2]; float* dgamma[2]; float* dbeta[2]; float* dalpha[2];
} CgCtxHeads;
int cg_context_heads_fwd(const CgCtxHeads* t, void* stream);
int cg_context_heads_bwd(const CgCtxHeads* t, void* stream);
long long cg_context_heads_red_doubles(int C);

/* ---- launch geometry queries (host only: no launch, no device access) ---------------------------------------------
 * What the launchers above would choose for a shape, answered by the very functions they call.  Most kernels hand a workgroup a
 * contiguous range of tiles / samples once the batch is large; tests ask here whether a shape really enters those loops.
 * Return value as everywhere (0 ok, -1 bad argument, -2 unsupported shape); `out` receives the ints listed.
 *   cg_map2adj_tail_geometry   one tower: out[4] = { positions per tile, tiles per sample, tiles per workgroup, workgroups per sample }
 *                              (workgroup ch of a sample walks tiles ch * tpw .. min(tiles, (ch + 1) * tpw) - 1; towers sharing a launch get
 *                              the larger workgroup count, the surplus workgroups return at once)
 *   cg_dstd_tail_geometry      out[12] = { samples per workgroup of the row phases, row workgroups per channel,
 *                              F2: positions per tile, tiles per sample, tiles, tiles per workgroup, workgroups,  K3: the same five }
 *                              (tiles in sample-major order; workgroup i walks tiles i * per .. min(total, (i + 1) * per) - 1)
 *   cg_pointwise_maps_geometry forward (bwd == 0) or backward: out[5] = { positions per tile, tiles per sample, tiles, tiles per workgroup,
 *                              workgroups }, ranges as above
 *   cg_collapse_geometry       backward of cg_collapse_rows (cols == 0) / cg_collapse_cols: out[3] = { K ranges, sample slices (grid y), samples
 *                              per slice }
 *   cg_fpn_conv_geometry       weight-gradient kernel: out[2] = { samples per workgroup, workgroups per dilation }
 *   cg_stgcn_domain_geometry   kind 0: tile kernels, kind 1: matrix-core kernels (stgcn_domain_mfma.hip); forward (bwd == 0) or backward:
 *                              out[6] = { tiles per sample, tiles, tiles per workgroup, workgroups, grid (workgroups rounded up to eight),
 *                              1 when this launch tries the plane kernels first (then the five numbers before describe the fall-back) }
 *   cg_block_input_geometry    out[3] = { planes (channels) per span, spans per sample, grid of the streaming kernels = B * spans } (a workgroup
 *                              owns one span of one sample; the last span of a sample is short when C is no multiple of the span)
 *   cg_norm_act_rows_per_block samples of one channel per workgroup of the row kernels (cg_norm_act_*, cg_chan_stats) for the view
 *   cg_glue_geometry           limits of the glue launchers and the plan of cg_dstd_stats_* for a (C,T,V) sample: out[11] = { points one grid of
 *                              cg_mpjpe_fwd covers, elements one grid of cg_adam_flat / cg_scale covers, bytes one grid of cg_zero covers (past
 *                              these a thread strides), largest C * H of the sliced cg_se_gate_bwd kernel (above it: one workgroup per
 *                              sample, atomics), its largest grid (more samples: a workgroup walks several), dynamic LDS bytes a kernel
 *                              gets without a raised limit, LDS bytes of cg_dstd_stats_bwd (-1: unsupported), lanes per row, rows per
 *                              iteration of a workgroup, iterations, rows of the last iteration } */
int cg_map2adj_tail_geometry(int B, int Kc, int J, int* out);
int cg_dstd_tail_geometry(int B, int C, int T, int V, int* out);
int cg_pointwise_maps_geometry(int B, int Cin, int P, int n, const int* M, int bwd, int* out);
int cg_collapse_geometry(int B, int C, int T, int V, int O, int cols, int* out);
int cg_fpn_conv_geometry(int B, int C, int O, int H, int W, int* out);
int cg_stgcn_domain_geometry(int B, int Cin, int Cout, int T, int V, int domain, int bwd, int kind, int* out);
int cg_block_input_geometry(int B, int C, int T, int V, int* out);
int cg_norm_act_rows_per_block(const CgView4* xv);
int cg_glue_geometry(int C, int T, int V, int* out);

/* ---- evaluation harness counterpart, environment/test.py:97-132 ----------------------
 * y[r,k,:] = x[r,idx[k],:] : `inputs[:, :, dim_used]` (32 -> 22 joints); x (rows,Jin,3), y (rows,Jout,3) contiguous */
int cg_gather_joints(const float* x, float* y, const int32_t* idx, long long rows, int Jin, int Jout, void* stream);
/* out = target with the prediction scattered back (`mygt[:, :, dim_used] = outputs`, repeated joints copied, test.py:121-127)
 * and frame_err[t] = mean over samples and joints of |out - target| (losses.mpjpe, reduce_axis (0,2), losses.py:50-61).
 * pred (B,To,J22,3), target/out (B,To,J32,3); src[j] = prediction joint taken by skeleton joint j, or -1 (ground truth kept) */
int cg_eval_scatter_mpjpe(const float* pred, const float* target, float* out, float* frame_err, const int32_t* src,
                          int B, int To, int J32, int J22, void* stream);

/* ---- on-device input pipeline -----------------------------------------------------------------
 * The training augmentations of environment/custom_transforms.py (RandomFlip :243-298, RandomRotation :10-84, RandomScale
 * :87-161, RandomNoise :350-400, RandomTranslation :164-240, RandomPoseInvers :301-347; order of loaders/loader.py:42-130) and
 * the per-item tensors of loaders/h36m_motion_3d.py:94-108 for a whole batch in one launch.  raw (B,L,J,3); params (B,24) = per
 * sequence [flip x,y,z | rotate? | R 3x3 row-major (p' = (p-c) R + c) | scale x,y,z | translation rate x,y,z | noise amplitude
 * (0: off) | invert? | pad], drawn on the host in the reference's order; noise_tab (B,J,3) the U(-1,1) draws of RandomNoise or
 * NULL; perm (J) the joint permutation the pair swaps of RandomPoseInvers compose to, or NULL; outputs sample (B,input_n,J,3),
 * target (B,L-input_n,J,3), target_vel (same shape, cumulative frame differences from frame input_n-1 on), target_gvel
 * (B,L-input_n,J,1) cumulative speeds, processed (B,L,J,3) or NULL, sample_vel (B,input_n,J,3) = frame differences of the input
 * frames or NULL (the same dictionary comes out of loaders/amass_motion_3d.py:76-91). */
int cg_augment_sequences(const float* raw, const float* params, float* sample, float* target, float* target_vel,
                         float* target_gvel, float* processed, float* sample_vel, const float* noise_tab, const int32_t* perm,
                         int B, int L, int J, int input_n, void* stream);

/* ---- robustness-test transforms (the `robustness_test:` section evaluate_robustness.py writes) ----------------------------------
 * The same transform classes with their `seq_idx`, `continuous` and `keep` arguments (environment/custom_transforms.py:
 * RandomRotation :50-78, RandomScale :127-153, RandomTranslation :202-231, RandomFlip :262-294, RandomPoseInvers :321-344,
 * RandomNoise :370-392), in the order loaders/loader.py:46-127 builds them, and the same per-item tensors as cg_augment_sequences
 * (loaders/h36m_motion_3d.py:94-108), for a whole batch in one launch.  The order of the transforms is data: the kernel executes
 * a list of up to CG_PERTURB_MAX_STEPS steps; a kind may occur more than once.
 *   steps     (n_steps,6) int on the HOST, the same for every sequence: [kind, s0, s1, continuous, keep, noise slot].  (A host
 *             table, copied into the launch: it is validated here without reading device memory, and the call stays capturable.)
 *   params    (B,n_steps,4) fp32 on the device: [apply?, v0, v1, v2] per sequence and step, drawn on the host in the reference's
 *             order.  v by kind - rotation: the rotation vector in DEGREES (the kernel does Rodrigues' formula itself, in f64, per
 *             frame); scale: the three factors; translation: the three rates; flip: per-axis 0/1; noise: the amplitude in v0;
 *             inversion: unused.
 *   noise_tab (B,n_noise,J,3) the U(-1,1) draws of RandomNoise, one slot per noise step (NULL when there is none)
 *   perm      (J) the joint permutation of RandomPoseInvers as in cg_augment_sequences (NULL when no step inverts)
 * A step owns the frame window [s0, s1), 0 <= s0 < s1 <= L ((0, L): the whole sequence).  With n = s1 - s0 its weight is
 *   f(t) = 0 for t < s0;  continuous ? (t - s0) / (n - 1) : 1 for s0 <= t < s1 (n == 1 and continuous: 0, as
 *   torch.linspace(0, v, 1) is [0]);  keep ? f(s1 - 1) : 0 for t >= s1.
 * Every step takes its centroid / extent from the WHOLE current sequence, frames outside its window included:
 *   rotation     p' = (p - c) R(t) + c, c the centroid of all L*J points, R(t) the matrix of the rotation vector f(t) * v (row-vector
 *                convention as above); frames with f(t) == 0 are not touched
 *   scale        p *= 1 + f(t) * (v - 1), about the origin (exactly v where f(t) == 1)
 *   translation  p += f(t) * v * ext, ext = per-axis max - min over the sequence before the step
 *   noise        p += f(t) * v0 * u[j][a] * ext[a]
 *   flip         no ramp: frames of [s0, s1), and with keep those from s1 on, are mirrored about the one centroid of the step's input
 *   inversion    no ramp: the joint permutation applies to frames [s0, s1), with keep to all frames >= s0.  It is applied while the
 *                results are written, so it must be the LAST step (where loader.py puts it)
 * With whole-sequence, non-continuous steps in the order flip, rotation, scale, noise, translation, inversion the results are
 * bit-identical to cg_augment_sequences (given the rotation matrix the host computes there).  raw is never written.
 * Returns -1 for a missing pointer (noise_tab / perm included when a step needs them), -2 for n_steps outside [0,
 * CG_PERTURB_MAX_STEPS], a window that is not 0 <= s0 < s1 <= L, an unknown kind, an inversion that is not the last step, a noise
 * slot outside [0, n_noise), or a sequence past the LDS bound of cg_augment_sequences (L*J*12 bytes <= 150 KiB).  n_steps == 0:
 * the untouched window and its item tensors. */
#define CG_PERTURB_MAX_STEPS 16
#define CG_PERTURB_ROTATION 0
#define CG_PERTURB_SCALE 1
#define CG_PERTURB_NOISE 2
#define CG_PERTURB_TRANSLATION 3
#define CG_PERTURB_FLIP 4
#define CG_PERTURB_INVERT 5
int cg_perturb_sequences(const float* raw, const int* steps, const float* params, const float* noise_tab, const int32_t* perm,
                         float* sample, float* target, float* target_vel, float* target_gvel, float* processed, float* sample_vel,
                         int B, int L, int J, int input_n, int n_steps, int n_noise, void* stream);

/* ---- optimizer on the flat parameter buffer -----------------------------------
 * torch.optim.Adam semantics (environment/utils.py:53-57): L2 weight decay added to the gradient,
 * bias-corrected moments; optional clip_grad_value_ (environment/train.py:97-98) and gradient
 * pre-scale (1/world_size after the RCCL all-reduce).  step_count is the 1-based step index. */
int cg_adam_flat(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, float lr, float beta1,
                 float beta2, float eps, float weight_decay, float grad_scale, float clip_value, long long step_count,
                 void* stream);

/* Gather (direction 0) / scatter (direction 1) between the 698 per-tensor gradient buffers and the
 * flat fp32 buffer that RCCL all-reduces: ptrs[t] <-> flat + flat_off[t], work pre-chunked
 * on the host (chunk i = chunk_len[i] elements of tensor chunk_tensor[i] from element chunk_begin[i]). */
int cg_multi_copy(void* ptrs, const long long* flat_off, const int32_t* chunk_tensor, const int32_t* chunk_begin,
                  const int32_t* chunk_len, int n_chunks, float* flat, int direction, float scale, void* stream);
/* `scale` multiplies the gathered gradients (direction 0): the replica weight B_r * world / sum B of a data-parallel step
 * with unequal per-GPU batches (BASELINE configs[4]); passing a sub-range of the chunk arrays gathers one bucket.
 * p[i] *= s: the 1/world of the gradient mean when no optimizer kernel follows to absorb it (cg_adam_flat's grad_scale). */
int cg_scale(float* p, long long n, float s, void* stream);

/* ---- input-space attacks (csrc/attack.hip) ----------------------------------------------------------
 * environment/adversarial_attacks.py of the reference.  An attack iteration is: eval-mode forward, one loss per sample
 * (`losses.mpjpe(..., reduce_axis=[1, 2])`, :175-178 with losses/losses.py:50-61), backward to the input poses, one step.
 * The reference re-slices the batch to the samples that are still optimised (`[op_mask]`, :518-521); here the batch keeps its
 * shape and a frozen sample has upstream weight 0, which gives the same signs and the same L1-normalised directions.
 * Per-sample MPJPE: pred / target contiguous (B,N,3), N = To*V; loss (B,), no atomics (bit-reproducible);
 * backward dpred[b] = w[b] * (pred - target) / (N * ||pred - target||), 0 where the norm is 0. */
int cg_mpjpe_sample_fwd(const float* pred, const float* tgt, float* loss, int B, int N, void* stream);
int cg_mpjpe_sample_bwd(const float* pred, const float* tgt, const float* w, float* dpred, int B, int N, void* stream);
/* One attack step, one workgroup per sample, everything of an iteration except the model call:
 *   mode 0 FGSM   (compute_gradient :401-417):  x = x + mask * eps_b * sign(grad); no reset, no bookkeeping
 *   mode 1 I-FGSM (:469-496):                   x = x + mask * (eps_b / iterations) * sign(grad)
 *   mode 2 MI-FGSM (:581-610):                  g = mu * g + grad / ||grad||_1 (per sample); x = x + mask * (eps_b / iterations) * sign(g)
 * with eps_b = epsilon * |max y - min y| of the CURRENT iterate (`_get_bound_per_sample`, typ_eval "len_y", :348-350).  Only samples
 * that are active at the start of the step move; then EVERY sample whose max |x - x0| exceeds eps_b has the elements outside
 * [x0 - eps_b, x0 + eps_b) reset to x0 (:486-493).  Bookkeeping of the active samples with loss[b] of this iteration (:517,
 * :529-538): queries += 1; best = loss if loss > best, else stall += 1; a sample with stall >= patience (5 in the reference) is
 * frozen: active = 0, w = 0, n_active -= 1; w = 1/B otherwise (the root gradient of the next backward).
 * A step that starts with every sample frozen changes nothing: the reference has left its loop by then (:540-541).  steps[b]
 * counts the steps of sample b and frozen_at[b] (INT_MAX while active) is the step at whose end it froze, so that every workgroup
 * can tell "active at the start of this step" apart from "frozen by another workgroup of this launch".
 * Deviation: an active sample whose gradient is all zero keeps g and x in MI-FGSM (the reference writes NaN there).
 * x is updated in place (x_i in, x_adv out); mask (T,V) of 0/1 or NULL; g only for mode 2; the bookkeeping pointers only for
 * modes 1 and 2.  T*V*3 <= cg_attack_step_max_floats() (the sample, x0 and the direction stay in LDS). */
typedef struct CgAttackStep {
  int B, T, V, mode, iterations, patience;
  float epsilon, mu;
  const float* x0;      /* (B,T,V,3) the clean input */
  float* x;             /* (B,T,V,3) in: x_i, out: x_adv (= the next x_i) */
  const float* grad;    /* (B,T,V,3) d(sum_b w_b loss_b)/dx_i */
  float* g;             /* (B,T,V,3) momentum (MI-FGSM only) */
  const float* mask;    /* (T,V) 1 = this joint of this frame may move; NULL = all */
  const float* loss;    /* (B,) loss_b of this iteration */
  float* best;          /* (B,) highest loss so far */
  int* stall;           /* (B,) iterations without improvement */
  int* active;          /* (B,) 1 while the sample is still optimised */
  float* w;             /* (B,) upstream weight of the NEXT backward: 1/B while active, else 0 */
  int* queries;         /* (B,) model calls spent on the sample */
  int* n_active;        /* (1,) samples still active (for the host to poll) */
  int* steps;           /* (B,) steps this sample has been through (each workgroup counts its own) */
  int* frozen_at;       /* (B,) index of the step at whose end the sample froze, INT_MAX while it is active */
} CgAttackStep;
int cg_attack_step(const CgAttackStep* a, void* stream);
long long cg_attack_step_max_floats(void);
/* One DeepFool step (DEEPFOOL.compute_gradient :697-717 with the bookkeeping of :755-767), one workgroup per sample:
 *   n1_b = ||grad_b||_1 + 1e-10;  r_b[t,v,c] = -grad_b[t,v,c] * mean_to(pred_b[to,v,c]) / n1_b;  x = x + mask * r
 * (`-(grad[:, None] * pred[:, :, None]).mean(1) / norm_grad`: the prediction's joints are broadcast onto the input's, so pred has the
 * V of x).  No epsilon, no reset.  The L1 norm and the To-means are accumulated in f64 in a fixed order, r is rounded to fp32 once;
 * no floating-point atomics, two calls give the same bits.  An all-zero gradient gives r = 0.  An element that does not move (frozen
 * sample, mask 0, r = 0) is not written, so a launch that starts with every sample frozen changes nothing but `steps`.
 * The bookkeeping is that of cg_attack_step on the same buffers; loss and the eight state pointers are given together, or all
 * NULL for a plain step of every sample.  mask (T,V) of 0/1 or NULL.  No shape limit: the To-means stay in LDS up to 4096 columns
 * (V*3) and are re-read per element beyond.  NULL x / grad / pred or a partial state: CG_EARG; a non-positive extent: CG_ESHAPE. */
typedef struct CgDeepfoolStep {
  int B, T, To, V, patience, pad;
  float* x;             /* (B,T,V,3) in: x_i, out: x_adv (= the next x_i) */
  const float* grad;    /* (B,T,V,3) d(sum_b w_b loss_b)/dx_i */
  const float* pred;    /* (B,To,V,3) the prediction of the same forward pass */
  const float* mask;    /* (T,V) 1 = this joint of this frame may move; NULL = all */
  const float* loss;    /* (B,) loss_b of this iteration; NULL (with the eight below) = no bookkeeping, every sample steps */
  float* best; int* stall; int* active; float* w; int* queries; int* n_active; int* steps; int* frozen_at;      /* as in CgAttackStep */
} CgDeepfoolStep;
int cg_deepfool_step(const CgDeepfoolStep* a, void* stream);

/* ---- evaluation metrics (csrc/eval_metrics.hip) ------------------------------------------------------
 * What environment/test.py::Metrics.compute (:65-94) reports per batch, except `mae`, in one pass on the device: out[] in the order
 *   0 mpjpe      losses.mpjpe (losses/losses.py:50-61)                    e = |P - X|
 *   1 pa_mpjpe   losses.pa_mpjpe (:79-144)                                |a P R + t - X| after the per-frame Procrustes fit, with the
 *                                                                         reference's replacement of centred target coordinates whose
 *                                                                         square is < 1e-6 by 1e-3 (:94), R = diag(1,1,sign det) V U^T
 *                                                                         (:106-119) and its NaN rule a -> 1, R -> 0, t -> 0 (:130-132)
 *   2 n_mpjpe    losses.n_mpjpe (:147-160)                                |c P - X|, c = mean_j(X.P) / mean_j(P.P) of the frame
 *   3 mve        losses.mean_velocity_error (:163-177)                    |(P[t+1] - P[t]) - (X[t+1] - X[t])|, To - 1 frames
 *   4 w_mpjpe    losses.weighted_mpjpe with temporal_w (:64-76, test.py:68,81)         w_t e, w_t = (t + 1) / To (test.py:301-302)
 *   5 bone_l     losses.bone_length_error (:199-215)                      | |P_i - P_j| - |X_i - X_j| | per bone (i,j)
 *   6 w_bone_l   losses.weighted_bone_length_error (:218-238)             w_t bone_l
 *   7 w_joints   losses.weighted_mpjpe with speeds (test.py:67,89)        sn e, sn = speeds / (max_j speeds + 1e-6)
 *   8 w_joints_t losses.weighted_mpjpe with speed_temporal_w (test.py:69-70,91)        (sn + w_t) / max_b(sn + w_t) e
 * frames = 1 (reduce_axis (0,2), test.py:289): every out[q] is (To,), the mean over samples and joints (bones), (To-1,) for mve;
 * frames = 0 (compute_joint_error, test.py:303-304): (B,To,J), (B,To-1,J) for mve, (B,To,Nb) for the bone metrics.
 * pred / target (B,To,J,3), speeds (B,To,J) contiguous and never written; bones (Nb,2) joint indices in [0,J);
 * J <= 64, To >= 2, Nb >= 1, B >= 1, else CG_ESHAPE.  ws: cg_eval_metrics_ws_doubles(B,To,J) doubles (0 for an unsupported shape).
 * No floating-point atomics (the sums over the batch are added in a fixed order): two calls give the same bits. */
#define CG_EM_METRICS 9
typedef struct CgEvalMetrics {
  int B, To, J, Nb, frames, pad;
  const float* pred; const float* target; const float* speeds; const int32_t* bones;
  float* out[CG_EM_METRICS];
  double* ws;               /* cg_eval_metrics_ws_doubles(B,To,J): [To*J] batch maxima | [7][B][To] per-frame sums */
} CgEvalMetrics;
int cg_eval_metrics(const CgEvalMetrics* a, void* stream);
long long cg_eval_metrics_ws_doubles(int B, int To, int J);

/* ---- attack distortion metrics (csrc/attack_metrics.hip) ---------------------------------------------
 * The numeric entries of the "adversarial_metrics" dictionary (environment/adversarial_attacks.py::ComputeAttackMetrics._get_metrics
 * :187-342, called as `_get_metrics(adv_inputs, inputs)` at environment/test.py:205): adv is the reference's `in_seq`, orig its `adv_seq`.
 * out[0..2] = mpjpe, n_mpjpe, pa_mpjpe (one value each, :192,:198,:204); then three families of ten, out[3 + 10 * family + q] with
 * family 0 temporal_* (T,), 1 spatial_* (J,), 2 *_sample (B,) and q in the order
 *   0 mpjpe          losses.mpjpe (losses/losses.py:50-61), |adv - orig|                          (:189-193)
 *   1 n_mpjpe        losses.n_mpjpe (:147-160), adv is `predicted`                               (:195-199)
 *   2 pa_mpjpe       losses.pa_mpjpe (:79-144), as in cg_eval_metrics                            (:201-205)
 *   3 hausdorff_mean HausdorffDistance("mean") (:106-147): min over the points of orig for every point of adv    (:212-214)
 *   4 hausdorff_max  HausdorffDistance("max")                                                    (:216-218)
 *   5 mse            nn.MSELoss(reduction='none')                                                (:232-234)
 *   6 cos_simil      nn.CosineSimilarity(eps=1e-6): over the flattened sample, else along the batch axis and averaged (:207-210)
 *   7 KLD            CustomKLD(bins=64) (:72-85), KL(adv || orig)                                (:220-222)
 *   8 JSD            CustomJSD(bins=64) (:55-69)                                                 (:224-226)
 *   9 KSTest         CustomKolmogorovSmirnovTest(bins=64) (:88-103)                              (:228-230)
 * The last three are over 64-bin density histograms of the joint-to-joint distances inside a frame (convert_to_dists :39-48), grouped
 * by sample, frame index or first joint; the 65 edges run from 0 to the group's maximum over both tensors, edge k = fl32(k / 64) * max
 * in fp32, and the binned distances carry the reference's fp32 bits.  A group whose maximum is 0 (all its joints coincide) gives NaN
 * in these three.  counts: int32 [2][B][CG_AM_BINS] | [2][T][CG_AM_BINS] | [2][J][CG_AM_BINS] (0 adv, 1 orig), zero-filled here; gmax: [B] | [T] | [J].
 * adv / orig contiguous and never written; B >= 1, T >= 1, 2 <= J <= 64, else CG_ESHAPE.  ws: cg_attack_metrics_ws_doubles(B,T,J)
 * doubles (0 for an unsupported shape).  No floating-point atomics: two calls give the same bits. */
#define CG_AM_OUT 33         /* 3 scalars + 3 families of ten */
#define CG_AM_BINS 64        /* bins of the density histograms */
typedef struct CgAttackMetrics {
  int B, T, J, pad;
  const float* adv; const float* orig;
  float* out[CG_AM_OUT];
  int32_t* counts; float* gmax;
  double* ws;
} CgAttackMetrics;
int cg_attack_metrics(const CgAttackMetrics* a, void* stream);
long long cg_attack_metrics_ws_doubles(int B, int T, int J);

/* ---- training losses other than plain MPJPE (csrc/losses.hip) -----------------------------------------
 * What `get_loss` (environment/train.py:15-43) selects by `learning_config.loss.type`, with the per-batch weights of train.py:62-71.
 * With d = pred - target per coordinate and e(b,t,v) the error of a joint, `kind` is
 *   CG_LOSS_WEIGHTED_MPJPE       losses.weighted_mpjpe (losses/losses.py:64-76)        e = |d|_2,  loss = mean(w e) over all B*T*V joints
 *                                                                                      (a plain mean: not divided by the sum of w)
 *   CG_LOSS_MPJPE_SOFT           losses.mpjpe_soft (:241-252)                          e = |s|_2, s_c = SmoothL1(d_c) with beta = 1
 *                                                                                      (0.5 d^2 if |d| < 1, else |d| - 0.5),  loss = mean(e)
 *   CG_LOSS_WEIGHTED_MPJPE_SOFT  losses.weighted_mpjpe_soft (:255-267)                 e as mpjpe_soft,  loss = mean(w e)
 *   CG_LOSS_RMPJPE               losses.rmpjpe (:36-47, reduce_axis=[])                e = |d|_2,  loss = sqrt(mean(e))
 * (plain `mpjpe` stays cg_mpjpe_fwd / cg_mpjpe_bwd).  The unweighted kinds ignore the weights, as the reference does.  The weight is
 *   w(b,t,v) = base(b,t,v) + speed_factor * speeds(b,t,v) / (max_v speeds(b,t,.) + 1e-6)
 * in fp32 and in the order of train.py:64-70: base = w_full[b,t,v] if w_full is given, else w_frame[t] if w_frame is given, else 0
 * (train.py:68, the weights string "speed"); the speed term is left out when speeds is NULL.  A weighted kind with none of the
 * three: CG_EARG.
 * Forward, two launches: one wavefront per (b,t) frame with the lanes over the joints (the frame maximum is a wave reduction; V > 64
 * loops), at most CG_LOSS_MAX_BLOCKS workgroups of CG_LOSS_THREADS that loop over the frames beyond one pass; each workgroup
 * leaves one f64 partial sum in `part`, a finishing launch adds them in a fixed order and stores `loss` and `mean` (the mean the
 * backward of rmpjpe needs).  No floating-point atomics: two calls give the same bits.
 * Backward, one launch: dpred = gloss[0] * dloss/dpred, gloss read from device memory; the frame maximum is recomputed.  target,
 * the weights and speeds get no gradient.  As torch: the gradient of a norm at 0 is 0 (a joint with e = 0 gets exact zeros),
 * SmoothL1' = d for |d| < 1, else sign(d); rmpjpe is gloss / (2 sqrt(mean)) times the gradient of the mean.
 * Deviations from the reference: (1) for mean = 0 torch's rmpjpe gradient is NaN, here it is 0; (2) every input is read-only - the
 * reference normalises `target_gvel` in place (`speeds /= ...` on a view of it, train.py:66), here speeds is never written.
 * pred / target (B,T,V,3), w_full / speeds (B,T,V), w_frame (T,), all contiguous; B, T, V >= 1 and kind one of the four, else CG_ESHAPE. */
#define CG_LOSS_WEIGHTED_MPJPE 0
#define CG_LOSS_MPJPE_SOFT 1
#define CG_LOSS_WEIGHTED_MPJPE_SOFT 2
#define CG_LOSS_RMPJPE 3
#define CG_LOSS_THREADS 256      /* per workgroup: CG_LOSS_THREADS / 64 frames in flight */
#define CG_LOSS_MAX_BLOCKS 512   /* workgroups of a launch = f64 words of `part` */
typedef struct CgMotionLoss {
  int kind, B, T, V;
  float speed_factor; int pad;
  const float* pred; const float* target;
  const float* w_full;      /* (B,T,V) or NULL */
  const float* w_frame;     /* (T,) or NULL; ignored when w_full is given */
  const float* speeds;      /* (B,T,V) or NULL */
  double* part;             /* forward scratch: CG_LOSS_MAX_BLOCKS doubles */
  float* loss;              /* forward out: one float */
  float* mean;              /* forward out, backward in: mean(e) resp. mean(w e), one float */
  const float* gloss;       /* backward in: the upstream gradient, one float */
  float* dpred;             /* backward out: (B,T,V,3) */
} CgMotionLoss;
int cg_motion_loss_fwd(const CgMotionLoss* a, void* stream);
int cg_motion_loss_bwd(const CgMotionLoss* a, void* stream);

/* ---- forward kinematics and the device-resident motion bank (csrc/kinematics.hip) -------------------------
 * What utils/data_utils.py::load_data_h36m (:843-942) and ::load_data_amass (:738-839) do before a window reaches a loader:
 * joint angles -> joint positions, one launch for all frames of a file.  The tree is data: parent[i] is the parent of joint i
 * (-1: a root; joint 0 must be one) with parent[i] < i for i >= 1, rest (J,3) the offsets (chain) / rest positions (SMPL),
 * select (J_out) the joints written (NULL: all J, in order), out (N,J_out,3) = scale * position.  `convention`:
 *   CG_FK_EXPMAP_CHAIN  utils/forward_kinematics.py::fkl_torch (:219-241) with data_utils.expmap2rotmat_torch (:1175-1194):
 *                       angles (N, 3 + 3J), joint i reads columns 3 + 3i .. 5 + 3i (the first three columns are ignored).
 *                       theta = |r|, r0 = r / (theta + 1e-7), K = skew(r0) (K[0][1] = -r0z, K[0][2] = r0y, K[1][2] = -r0x),
 *                       R_i = I + sin(theta) K + (1 - cos(theta)) K^2; p_i = rest_i; then for i >= 1 in index order and ONLY IF
 *                       parent[i] > 0:  R_i = R_i R_parent,  p_i = rest_i R_parent + p_parent (row vector times matrix).
 *                       A joint whose parent is joint 0 (or that has none) keeps its local rotation and p = rest - joint 0's own
 *                       rotation never reaches anything.  That is the reference's `if parent[i] > 0` and not the usual recursion;
 *                       what its loaders emit depends on it, so it is reproduced.
 *   CG_FK_SMPL          utils/ang2joint.py::ang2joint (:11-58) with rodrigues (:64-91): angles = pose (N, J_pose, 3), J_pose >= J,
 *                       the first J joints are read.  theta = |r|, k = r / theta, R = cos(theta) I + (1 - cos(theta)) k k^T +
 *                       sin(theta) skew(k); G_i = G_parent [R_i | rest_i - rest_parent] (a root: [R_i | rest_i]); the position is
 *                       the translation of G_i.  The reference adds N(0, 1e-8) noise to r before the norm so that theta != 0;
 *                       nothing is drawn here: theta = |r| and theta == 0 gives R = I exactly, the reference's result for r = 0.
 * The kernel reads fp32, composes in f64 and rounds each coordinate to fp32 once; angles, rest and the tables are never written,
 * nothing is accumulated with atomics: two calls give the same bits.  One lane per joint, two frames per wavefront while J and
 * J_out <= 32, the frame's global rotations and positions in LDS, one pass per tree level; at most CG_FK_MAX_BLOCKS workgroups,
 * each walking the frame groups beyond one pass, so N is not bounded.
 * `parent` is a HOST array (like the step table of cg_perturb_sequences it is validated here without reading device memory and
 * copied into the launch; the call stays capturable); every other pointer is a device pointer.
 * Returns -1 for a missing angles / parent / rest / out; -2 for J or J_out outside [1, CG_FK_MAX_JOINTS], an unknown convention,
 * J_pose < J (SMPL), N < 0, parent[0] != -1 or a parent[i] outside [-1, i).  An entry of `select` outside [0, J) is clamped into
 * it (the host path raises first).  N == 0: nothing is launched. */
#define CG_FK_MAX_JOINTS 64
#define CG_FK_MAX_BLOCKS 1024    /* workgroups of a launch; one holds CG_FK_THREADS / 64 wavefronts of one or two frames */
#define CG_FK_THREADS 256
#define CG_FK_EXPMAP_CHAIN 0
#define CG_FK_SMPL 1
typedef struct CgForwardKinematics {
  int convention, J, J_pose, J_out;   /* J_pose: joints per input row (SMPL; ignored by the chain convention) */
  long long N;                        /* frames */
  float scale; int pad;
  const float* angles;                /* (N, 3 + 3J) | (N, J_pose, 3) */
  const int* parent;                  /* HOST (J) */
  const float* rest;                  /* (J,3) */
  const int32_t* select;              /* (J_out) or NULL (then J_out == J) */
  float* out;                         /* (N, J_out, 3) */
} CgForwardKinematics;
int cg_forward_kinematics(const CgForwardKinematics* a, void* stream);

/* One batch of sliding windows cut out of a bank of distinct frames: `the_sequence[fs_sel]` (data_utils.py:891-896, :812-817),
 * `self.target[:, :, dim_used]` and `(all_seqs - data_mean) / data_std` (loaders/h36m_motion_3d.py:62-68) and the pose-inversion fix
 * of H36m_Motion3D.__init__ (:70-74 with :79-89), for the windows a batch names - the (n, seq_len, J, 3) array of every window is
 * never built.  frames (F,J_src,3); starts (W) the first frame of every window; items (B) window ids; raw (B,L,J,3):
 *   raw[b,t,j,:] = (frames[starts[items[b]] + t, select[j], :] - mean) / std        (fp32; mean 0 and std 1: the bits of frames)
 * Inversion check (up_hi, up_lo >= 0, joints in the SELECTED numbering - the loader's head and hip): a window with
 * y[0, up_hi] - y[0, up_lo] < 0 (strictly, in fp32, as `np.sign(...) == -1`) has y := c - y on every frame, c the mean of its L*J
 * normalised y values accumulated in f64 in a fixed order and rounded to fp32 once (the reference takes an fp32 mean).  Both -1: off.
 * One workgroup per window; no atomics, two calls give the same bits; frames, starts and items are never written.
 * items[b] is clamped into [0, W) and starts[.] into [0, F - L], an entry of select into [0, J_src): a bad id cannot read out of
 * bounds (the host path validates and raises first).
 * Returns -1 for a missing frames / starts / items / raw; -2 for B, L, J, J_src or W < 1, F < L, std == 0, select == NULL with
 * J != J_src, or up_hi / up_lo that are neither both -1 nor both in [0, J). */
typedef struct CgGatherWindows {
  int B, L, J_src, J, W, up_hi, up_lo, pad;
  long long F;
  float mean, std;
  const float* frames; const int32_t* starts; const int32_t* items; const int32_t* select;
  float* raw;
} CgGatherWindows;
int cg_gather_windows(const CgGatherWindows* a, void* stream);
/* The same gather with the window ids read at a device-resident cursor, so that a captured step takes the next batch of an epoch
 * without the host naming it: window id b is order[min(*cursor + b, W - 1)] (then clamped as items[b] is).  order (W) and cursor (1)
 * are device pointers, a->items is ignored (it may be NULL); everything else, the return codes included, as cg_gather_windows, with
 * -1 for a missing order / cursor.  A cursor past W - B repeats window order[W - 1] instead of reading out of bounds; a negative
 * one is taken as 0. */
int cg_gather_windows_at(const CgGatherWindows* a, const int32_t* order, const int32_t* cursor, void* stream);
/* *cursor += by: one thread, a plain vector store (like cg_seed_bump), so that the cursor moves inside a captured step */
int cg_cursor_advance(int32_t* cursor, int by, void* stream);

/* ---- the random draws of the augmentations on the device (csrc/augment_draw.hip) ---------------------------------------------
 * Fills the parameter table cg_augment_sequences / cg_perturb_sequences read from the device-resident seed word of the dropout
 * (cg_seed_bump advances it), so that a captured step draws its own augmentations.  This is a different random stream than the
 * host draws of environment/input_pipeline.py, which reproduce the reference's np.random order.
 *   steps   n_steps descriptors on the HOST (copied into the launch: validated without reading device memory, the call stays
 *           capturable), kind = a CG_PERTURB_* code.  rotation / scale / translation: the amounts are drawn from [lo[a], hi[a]];
 *           flip: lo[a] != 0 marks an enabled axis; noise: the amplitude is lo[0]; inversion: nothing else.
 *   seed    the device seed word, read and never written;  stream_id 0 .. 65535 separates independent draws under one seed
 * Generator (the specification a test restates):
 *   bits = splitmix64 finaliser of (seed, salt, counter), the dropout hash:
 *            z = counter + seed * 0x9E3779B97F4A7C15 + (salt << 40) + 0x632BE59BD9B4E019   (mod 2^64)
 *            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  bits = z ^ (z >> 31)
 *   u = (bits >> 40) * 2^-24, in [0, 1) and exact in fp32
 *   parameters  salt = CG_DRAW_SALT + stream_id, counter = (b * n_steps + step) * 4 + slot; slot 0 is the coin of the step, slots
 *               1 - 3 its three amounts; a flip has the coins of x, y, z in slots 0 - 2 and draws only for its enabled axes
 *   noise       salt = CG_DRAW_SALT + 0x10000 + stream_id, counter = ((b * n_noise + noise_slot) * J + j) * 3 + axis, value = 2 u - 1;
 *               noise_slot counts the noise steps of the list in order; drawn whether or not the step's coin says 'apply'
 *   a step applies iff u > prob_threshold (fp32 comparison; `rng.uniform() > thr` of the reference)
 *   amount = lo + (hi - lo) * u in f64 from the fp32 bounds, rounded to fp32 once
 * The counters are fixed: unlike the host path no draw depends on the outcome of another.  Dropout site ids share the salt field
 * and stay below CG_DRAW_SALT (the model asserts it).
 * Outputs (device):
 *   layout CG_DRAW_TABLE24  table (B,24), the row of cg_augment_sequences: flips 0-2, rotate? 3, R row-major 4-12 (Rodrigues'
 *                           formula in f64 on the drawn fp32 degrees, rounded once), scale 13-15, translation 16-18, noise
 *                           amplitude 19, invert? 20, 21-23 zero.  A step that does not apply - and a kind the list does not hold -
 *                           leaves the identity: scale 1, everything else 0.  Of a kind that occurs more than once the LAST step
 *                           fills the columns (the others are drawn and dropped).
 *   layout CG_DRAW_STEPS4   table (B,n_steps,4), the rows [apply?, v0, v1, v2] of cg_perturb_sequences: rotation in degrees, scale
 *                           factors, translation rates, noise [1, amplitude, 0, 0], inversion [1, 0, 0, 0], flip [OR of the axes,
 *                           x, y, z]; all four 0 when the step does not apply.  n_steps == 0: nothing to write.
 *   noise_tab (B,n_noise,J,3) U(-1,1), with either layout, when the list holds noise steps
 * One thread per (sample, step) and one per noise element (grid-stride past CG_DRAW_MAX_BLOCKS workgroups of CG_DRAW_THREADS);
 * no atomics: two calls under the same seed give the same bits.
 * Returns -1 for a missing seed / table / steps (n_steps > 0); -2 for B < 1, n_steps outside [0, CG_PERTURB_MAX_STEPS], an
 * unknown kind or layout, stream_id outside [0, 65535], or a noise step with J < 1 or without noise_tab. */
#define CG_DRAW_SALT 0x800000
#define CG_DRAW_TABLE24 0
#define CG_DRAW_STEPS4 1
#define CG_DRAW_THREADS 256
#define CG_DRAW_MAX_BLOCKS 4096
typedef struct CgDrawStep { int kind; float prob_threshold; float lo[3]; float hi[3]; } CgDrawStep;
int cg_draw_augmentation(const CgDrawStep* steps, int n_steps, const unsigned long long* seed, int stream_id, int B, int J, int layout,
                         float* table, float* noise_tab, void* stream);

#ifdef __cplusplus
}
#endif
#endif
