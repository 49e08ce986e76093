// creditcore HIP kernels — gfx950 (MI355X) native scoring hot path.
//
// Replaces the reference's CPU hot loops (sklearn RF predict_proba,
// alibi-detect IForest.predict and TabularDrift.predict, invoked per request
// at /root/reference/databricks/src/02-register-model.ipynb cell-9 via
// app/main.py:72) with CDNA4 kernels over the flat buffers produced by
// creditcore/pack.py:
//
//   forest_kernel    — node-SoA BFS forest traversal (classifier + iforest).
//                      One thread per (row, tree-chunk); per-row features are
//                      staged in LDS column-major so the divergent, dynamically
//                      indexed feature lookups hit LDS instead of scratch.
//                      Leaf sums accumulate in f64 (one atomicAdd per thread)
//                      for bit-stable parity with the f64 CPU reference.
//   finalize_kernel  — P(default) = acc/n_trees; isolation-forest anomaly
//                      score 2^(-depth/denom) + offset and outlier threshold.
//   cat_hist_kernel  — per-categorical-feature batch histograms (LDS-partial,
//                      one global atomicAdd per non-zero bin per block).
//   ks_kernel        — exact two-sample K-S D per numeric feature: bitonic
//                      sort of the batch column in LDS, then per-element
//                      binary search into the sorted reference (L2-resident)
//                      evaluating |F_ref - F_batch| at both one-sided limits.
//
// Design notes (MI355X): wavefront = 64; block = 256 (4 waves); grids are
// sized ≥ ~2048 blocks where the batch allows so all 256 CUs across the
// 8 XCDs see work; everything stays on the caller's HIP stream (the engine's
// private per-replica stream) — no host sync inside.

#include <torch/extension.h>

#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#define BLOCK 256
#define N_CAT 9
#define N_NUM 14
#define MAX_DRIFT_ROWS 16384  // LDS cap for the K-S sort (64 KiB of f32)
static constexpr size_t KS_LDS_BYTES_MAX = 160 * 1024 - 1024;  // gfx950 LDS/CU

#define HIP_CHECK(expr)                                              \
  do {                                                               \
    hipError_t _e = (expr);                                          \
    TORCH_CHECK(_e == hipSuccess, "HIP error: ", hipGetErrorString(_e)); \
  } while (0)

// ---------------------------------------------------------------------------
// Forest traversal
// ---------------------------------------------------------------------------

// DIRECT=false: classifier — node.feat is a virtual feature resolved through
//   feat_col/feat_code (one-hot membership test or numeric passthrough).
// DIRECT=true: isolation forest — node.feat indexes the numeric columns.
template <bool DIRECT>
__global__ __launch_bounds__(BLOCK) void forest_kernel(
    const short* __restrict__ codes,    // [B, N_CAT]
    const float* __restrict__ nums,     // [B, N_NUM]
    const float* __restrict__ medians,  // [N_NUM]
    const int4* __restrict__ nodes,     // [n_nodes] {feat, bits, left, right}
    const int* __restrict__ tree_off,   // [T+1]
    int n_trees,
    const int* __restrict__ feat_col,   // [F] (unused when DIRECT)
    const int* __restrict__ feat_code,  // [F] (unused when DIRECT)
    int n_rows,
    double* __restrict__ acc)           // [B], pre-zeroed
{
  // Column-major LDS staging: lane-consecutive addresses per column access
  // are stride-1 → conflict-free; dynamic per-node column indexing stays in
  // LDS instead of spilling a register-indexed array to scratch.
  __shared__ short s_codes[N_CAT * BLOCK];
  __shared__ float s_nums[N_NUM * BLOCK];

  const int tid = threadIdx.x;
  const int row = blockIdx.x * BLOCK + tid;
  if (row < n_rows) {
    if (!DIRECT) {
#pragma unroll
      for (int c = 0; c < N_CAT; ++c) s_codes[c * BLOCK + tid] = codes[row * N_CAT + c];
    }
#pragma unroll
    for (int c = 0; c < N_NUM; ++c) {
      const float v = nums[row * N_NUM + c];
      s_nums[c * BLOCK + tid] = isnan(v) ? medians[c] : v;  // fused imputation
    }
  }
  // No __syncthreads(): each thread only reads its own LDS slots.
  if (row >= n_rows) return;

  double local = 0.0;
  for (int t = blockIdx.y; t < n_trees; t += gridDim.y) {
    const int base = tree_off[t];
    int4 nd = nodes[base];
    while (nd.x >= 0) {
      float v;
      if (DIRECT) {
        v = s_nums[nd.x * BLOCK + tid];
      } else {
        const int col = feat_col[nd.x];
        const int code = feat_code[nd.x];
        v = (code >= 0) ? ((s_codes[col * BLOCK + tid] == (short)code) ? 1.0f : 0.0f)
                        : s_nums[col * BLOCK + tid];
      }
      const float thr = __int_as_float(nd.y);
      nd = nodes[base + ((v <= thr) ? nd.z : nd.w)];
    }
    local += (double)__int_as_float(nd.y);  // leaf payload
  }
  atomicAdd(&acc[row], local);
}

// ILP variant: each thread walks TWO trees concurrently — two independent
// node-gather chains per lane double the memory-level parallelism of the
// latency-bound traversal (A/B'd against forest_kernel via kernel_micro).
template <bool DIRECT>
__global__ __launch_bounds__(BLOCK) void forest_kernel_ilp(
    const short* __restrict__ codes,
    const float* __restrict__ nums,
    const float* __restrict__ medians,
    const int4* __restrict__ nodes,
    const int* __restrict__ tree_off,
    int n_trees,
    const int* __restrict__ feat_col,
    const int* __restrict__ feat_code,
    int n_rows,
    double* __restrict__ acc)
{
  __shared__ short s_codes[N_CAT * BLOCK];
  __shared__ float s_nums[N_NUM * BLOCK];
  const int tid = threadIdx.x;
  const int row = blockIdx.x * BLOCK + tid;
  if (row < n_rows) {
    if (!DIRECT) {
#pragma unroll
      for (int c = 0; c < N_CAT; ++c) s_codes[c * BLOCK + tid] = codes[row * N_CAT + c];
    }
#pragma unroll
    for (int c = 0; c < N_NUM; ++c) {
      const float v = nums[row * N_NUM + c];
      s_nums[c * BLOCK + tid] = isnan(v) ? medians[c] : v;
    }
  }
  if (row >= n_rows) return;

  auto value_of = [&](int f) -> float {
    if (DIRECT) return s_nums[f * BLOCK + tid];
    const int col = feat_col[f];
    const int code = feat_code[f];
    return (code >= 0) ? ((s_codes[col * BLOCK + tid] == (short)code) ? 1.0f : 0.0f)
                       : s_nums[col * BLOCK + tid];
  };

  double local = 0.0;
  for (int t = blockIdx.y; t < n_trees; t += 2 * gridDim.y) {
    const int ta = t;
    const int tb = t + gridDim.y;
    const int basea = tree_off[ta];
    int4 na = nodes[basea];
    bool la = true;
    int baseb = 0;
    int4 nb;
    bool lb = tb < n_trees;
    if (lb) { baseb = tree_off[tb]; nb = nodes[baseb]; }
    while (la || lb) {
      if (la) {
        if (na.x >= 0) {
          const float v = value_of(na.x);
          na = nodes[basea + ((v <= __int_as_float(na.y)) ? na.z : na.w)];
        } else {
          local += (double)__int_as_float(na.y);
          la = false;
        }
      }
      if (lb) {
        if (nb.x >= 0) {
          const float v = value_of(nb.x);
          nb = nodes[baseb + ((v <= __int_as_float(nb.y)) ? nb.z : nb.w)];
        } else {
          local += (double)__int_as_float(nb.y);
          lb = false;
        }
      }
    }
  }
  atomicAdd(&acc[row], local);
}

// Dual-forest fusion: classifier (one-hot resolution) and isolation forest
// (direct numeric features) in ONE launch — grid-y is split into
// chunks_cls classifier chunks followed by iforest chunks, each block
// running the same 2-tree-ILP walk against its forest's tables. The two
// forests were two serial launches in round 1 (~9.4 µs of iforest after
// ~33 µs of classifier at b=1024); one grid lets the scheduler run both
// concurrently with NO new graph edges (a 3-stream fork was measured
// SLOWER — the extra cross-stream edges cost ~20 µs/replay, see
// kernel_tuning.md).
template <bool DIRECT>
__device__ __forceinline__ double forest_walk_ilp2(
    const short* __restrict__ s_codes,
    const float* __restrict__ s_nums,
    int tid,
    const int4* __restrict__ nodes,
    const int* __restrict__ tree_off,
    int n_trees,
    const int* __restrict__ feat_col,
    const int* __restrict__ feat_code,
    int chunk,
    int n_chunks)
{
  auto value_of = [&](int f) -> float {
    if (DIRECT) return s_nums[f * BLOCK + tid];
    const int col = feat_col[f];
    const int code = feat_code[f];
    return (code >= 0) ? ((s_codes[col * BLOCK + tid] == (short)code) ? 1.0f : 0.0f)
                       : s_nums[col * BLOCK + tid];
  };
  double local = 0.0;
  for (int t = chunk; t < n_trees; t += 2 * n_chunks) {
    const int ta = t;
    const int tb = t + n_chunks;
    const int basea = tree_off[ta];
    int4 na = nodes[basea];
    bool la = true;
    int baseb = 0;
    int4 nb;
    bool lb = tb < n_trees;
    if (lb) { baseb = tree_off[tb]; nb = nodes[baseb]; }
    while (la || lb) {
      if (la) {
        if (na.x >= 0) {
          const float v = value_of(na.x);
          na = nodes[basea + ((v <= __int_as_float(na.y)) ? na.z : na.w)];
        } else {
          local += (double)__int_as_float(na.y);
          la = false;
        }
      }
      if (lb) {
        if (nb.x >= 0) {
          const float v = value_of(nb.x);
          nb = nodes[baseb + ((v <= __int_as_float(nb.y)) ? nb.z : nb.w)];
        } else {
          local += (double)__int_as_float(nb.y);
          lb = false;
        }
      }
    }
  }
  return local;
}

__global__ __launch_bounds__(BLOCK) void forest_kernel_dual(
    const short* __restrict__ codes,
    const float* __restrict__ nums,
    const float* __restrict__ medians,
    const int4* __restrict__ cls_nodes,
    const int* __restrict__ cls_off,
    int t_cls,
    const int* __restrict__ feat_col,
    const int* __restrict__ feat_code,
    const int4* __restrict__ if_nodes,
    const int* __restrict__ if_off,
    int t_if,
    int chunks_cls,
    int n_rows,
    double* __restrict__ acc_cls,
    double* __restrict__ acc_if)
{
  __shared__ short s_codes[N_CAT * BLOCK];
  __shared__ float s_nums[N_NUM * BLOCK];
  const int tid = threadIdx.x;
  const int row = blockIdx.x * BLOCK + tid;
  const bool is_cls = (int)blockIdx.y < chunks_cls;
  if (row < n_rows) {
    if (is_cls) {
#pragma unroll
      for (int c = 0; c < N_CAT; ++c) s_codes[c * BLOCK + tid] = codes[row * N_CAT + c];
    }
#pragma unroll
    for (int c = 0; c < N_NUM; ++c) {
      const float v = nums[row * N_NUM + c];
      s_nums[c * BLOCK + tid] = isnan(v) ? medians[c] : v;
    }
  }
  if (row >= n_rows) return;
  if (is_cls) {
    const double local = forest_walk_ilp2<false>(
        s_codes, s_nums, tid, cls_nodes, cls_off, t_cls, feat_col, feat_code,
        blockIdx.y, chunks_cls);
    atomicAdd(&acc_cls[row], local);
  } else {
    const double local = forest_walk_ilp2<true>(
        s_codes, s_nums, tid, if_nodes, if_off, t_if, nullptr, nullptr,
        blockIdx.y - chunks_cls, gridDim.y - chunks_cls);
    atomicAdd(&acc_if[row], local);
  }
}

// Per-row feature attributions ("reason codes") for the classifier forest:
// the prediction-path (Saabas) decomposition. A second walk over the same
// nodes as forest_kernel<false> that, at every split, credits
// v[child taken] - v[node] (v = cover-weighted expected value per node,
// pack.py cls_node_value) to the SOURCE column of the split feature — one-hot
// virtual features fold back onto their categorical column, numeric feature
// j lands in column N_CAT + j. base + sum_c contrib[row, c] telescopes to the
// model output.
//
// Same grid idea as forest_kernel (one thread per (row, tree-chunk), rows
// staged in LDS column-major with fused imputation). The N_SRC per-thread
// f64 accumulators are indexed by a runtime column, so they live in LDS
// column-major (a register array would go to scratch); each thread touches
// only its own slots — no barrier, no LDS atomics.
//
// LDS budget: this kernel runs 128-thread blocks (CONTRIB_BLOCK, NOT BLOCK):
// 23*128*8 B accumulators + 9*128*2 B codes + 14*128*4 B nums = 33,024 B
// static, under the 64 KiB static limit with several blocks per CU. At 256
// threads the accumulators alone would need 47 KiB and the total 66 KiB.
// The walk is one tree at a time: one extra 4-byte gather per step (the
// child's value; the current node's value is carried along).
#define CONTRIB_BLOCK 128
#define N_SRC (N_CAT + N_NUM)

__global__ __launch_bounds__(CONTRIB_BLOCK) void forest_contrib_kernel(
    const short* __restrict__ codes,       // [B, N_CAT]
    const float* __restrict__ nums,        // [B, N_NUM]
    const float* __restrict__ medians,     // [N_NUM]
    const int4* __restrict__ nodes,        // [n_nodes] {feat, bits, left, right}
    const float* __restrict__ node_value,  // [n_nodes]
    const int* __restrict__ tree_off,      // [T+1]
    int n_trees,
    const int* __restrict__ feat_col,      // [F]
    const int* __restrict__ feat_code,     // [F]
    int n_rows,
    double scale,                          // 1/T (averaging forest) or 1 (GBT)
    double* __restrict__ contrib)          // [B, N_SRC], pre-zeroed
{
  __shared__ double s_acc[N_SRC * CONTRIB_BLOCK];
  __shared__ short s_codes[N_CAT * CONTRIB_BLOCK];
  __shared__ float s_nums[N_NUM * CONTRIB_BLOCK];

  const int tid = threadIdx.x;
  const int row = blockIdx.x * CONTRIB_BLOCK + tid;
  if (row >= n_rows) return;  // no barrier below: own LDS slots only

#pragma unroll
  for (int c = 0; c < N_CAT; ++c)
    s_codes[c * CONTRIB_BLOCK + tid] = codes[(size_t)row * N_CAT + c];
#pragma unroll
  for (int c = 0; c < N_NUM; ++c) {
    const float v = nums[(size_t)row * N_NUM + c];
    s_nums[c * CONTRIB_BLOCK + tid] = isnan(v) ? medians[c] : v;
  }
#pragma unroll
  for (int c = 0; c < N_SRC; ++c) s_acc[c * CONTRIB_BLOCK + tid] = 0.0;

  for (int t = blockIdx.y; t < n_trees; t += gridDim.y) {
    const int base = tree_off[t];
    int4 nd = nodes[base];
    float v_cur = node_value[base];
    while (nd.x >= 0) {
      const int col = feat_col[nd.x];
      const int code = feat_code[nd.x];
      const float v =
          (code >= 0) ? ((s_codes[col * CONTRIB_BLOCK + tid] == (short)code) ? 1.0f : 0.0f)
                      : s_nums[col * CONTRIB_BLOCK + tid];
      const int next = base + ((v <= __int_as_float(nd.y)) ? nd.z : nd.w);
      nd = nodes[next];
      const float v_next = node_value[next];
      const int src = (code >= 0) ? col : (N_CAT + col);
      s_acc[src * CONTRIB_BLOCK + tid] += (double)v_next - (double)v_cur;
      v_cur = v_next;
    }
  }

  double* out = contrib + (size_t)row * N_SRC;
#pragma unroll
  for (int c = 0; c < N_SRC; ++c) {
    const double a = s_acc[c * CONTRIB_BLOCK + tid];
    if (a != 0.0) atomicAdd(&out[c], a * scale);
  }
}

// Exact path-dependent TreeSHAP over the flat path table of pack.py
// (build_shap_paths). For one leaf with value v and distinct players p on its
// path (z_p = product of cover fractions over p's splits, o_p = 1 iff the row
// follows all of them):
//
//   phi_i = v (o_i - z_i) * int_0^1 prod_{p != i} (z_p (1-t) + o_p t) dt
//
// The integrand has degree <= N_SRC - 2, so the SHAP_NQ-point Gauss-Legendre
// rule is exact. With f_pq = z_p + (o_p - z_p) t_q and L_q = prod_p f_pq,
// player i gets v (o_i - z_i) sum_q w_q L_q / f_iq:
//   o_i = 0: f_iq = z_i (1 - t_q), z_i cancels: phi_i = -v sum_q w_q/(1-t_q) L_q
//            (the same sum for every such player of the leaf; no division);
//   o_i = 1: 1/f_iq depends on the path only, not on the row. The block
//            computes those reciprocals once per path into LDS (one division
//            per thread) and every row multiplies.
//
// forest_contrib_kernel's skeleton: one thread per row, CONTRIB_BLOCK rows
// staged column-major in LDS with fused imputation, N_SRC f64 accumulators
// per thread in LDS, blockIdx.y strides over paths. All threads of a block
// work on the same path, so record loads are block-uniform and every loop has
// a uniform trip count (the barriers below rely on that: threads past n_rows
// stay in the loops on a clamped row and only skip the flush).
// LDS: 33,024 B as forest_contrib_kernel + 2,208 B reciprocals + 464 B.
#define SHAP_NQ 12
static_assert(2 * SHAP_NQ >= N_SRC, "Gauss-Legendre rule too small for N_SRC players");

#define SHAP_DIR_RIGHT 1
#define SHAP_FIRST 2
#define SHAP_PLAYER_SHIFT 8
#define SHAP_CODE_SHIFT 16

// Gauss-Legendre nodes t_q and weights w_q on [0, 1], and w_q / (1 - t_q)
#define SHAP_T_LIST                                                         \
  0.009219682876640378, 0.0479413718147626, 0.11504866290284765,            \
  0.20634102285669126, 0.31608425050090994, 0.43738329574426554,            \
  0.5626167042557344, 0.6839157494990901, 0.7936589771433087,               \
  0.8849513370971523, 0.9520586281852375, 0.9907803171233596
#define SHAP_W_LIST                                                         \
  0.02358766819325601, 0.05346966299765944, 0.08003916427167306,            \
  0.10158371336153282, 0.11674626826917732, 0.12457352290670134,            \
  0.12457352290670134, 0.11674626826917732, 0.10158371336153282,            \
  0.08003916427167306, 0.05346966299765944, 0.02358766819325601

__global__ __launch_bounds__(CONTRIB_BLOCK) void forest_shap_kernel(
    const short* __restrict__ codes,       // [B, N_CAT]
    const float* __restrict__ nums,        // [B, N_NUM]
    const float* __restrict__ medians,     // [N_NUM]
    const float* __restrict__ leaf_value,  // [L]
    const int* __restrict__ leaf_off,      // [L+1] into splits
    const int4* __restrict__ splits,       // [S] {feat, thr bits, frac bits, flags}
    int n_leaves,
    int n_rows,
    double scale,                          // 1/T (averaging forest) or 1 (GBT)
    double* __restrict__ shap)             // [B, N_SRC], pre-zeroed
{
  constexpr double T[SHAP_NQ] = {SHAP_T_LIST};
  constexpr double W[SHAP_NQ] = {SHAP_W_LIST};

  __shared__ double s_acc[N_SRC * CONTRIB_BLOCK];
  __shared__ short s_codes[N_CAT * CONTRIB_BLOCK];
  __shared__ float s_nums[N_NUM * CONTRIB_BLOCK];
  __shared__ double s_rcp[N_SRC * SHAP_NQ];  // 1 / f_pq for o_p = 1
  // z_p per player group of the path. Two buffers by path parity: pass 2 of
  // one path reads it while thread 0 may already write the next path's.
  __shared__ double s_z[2][N_SRC];
  __shared__ double s_t[SHAP_NQ];

  const int tid = threadIdx.x;
  const int row_raw = blockIdx.x * CONTRIB_BLOCK + tid;
  const bool live = row_raw < n_rows;
  const int row = live ? row_raw : n_rows - 1;  // n_rows >= 1 (host)

#pragma unroll
  for (int c = 0; c < N_CAT; ++c)
    s_codes[c * CONTRIB_BLOCK + tid] = codes[(size_t)row * N_CAT + c];
#pragma unroll
  for (int c = 0; c < N_NUM; ++c) {
    const float v = nums[(size_t)row * N_NUM + c];
    s_nums[c * CONTRIB_BLOCK + tid] = isnan(v) ? medians[c] : v;
  }
#pragma unroll
  for (int c = 0; c < N_SRC; ++c) s_acc[c * CONTRIB_BLOCK + tid] = 0.0;
#pragma unroll
  for (int q = 0; q < SHAP_NQ; ++q)
    if (tid == q) s_t[q] = T[q];

  int par = 0;
  for (int leaf = blockIdx.y; leaf < n_leaves; leaf += gridDim.y) {
    const int r0 = leaf_off[leaf];
    const int r1 = leaf_off[leaf + 1];
    if (r1 == r0) continue;  // root leaf: no players (block-uniform)
    par ^= 1;
    double* sz = s_z[par];

    // pass 1: which player groups the row follows, z_p, and L_q
    double L[SHAP_NQ];
#pragma unroll
    for (int q = 0; q < SHAP_NQ; ++q) L[q] = 1.0;
    unsigned omask = 0;
    int m = 0;  // player groups closed so far
    double z = 1.0;
    bool o = true;
    for (int r = r0; r < r1; ++r) {
      const int4 rec = splits[r];
      const int player = (rec.w >> SHAP_PLAYER_SHIFT) & 0xFF;
      const int code = (int)((unsigned)rec.w >> SHAP_CODE_SHIFT) - 1;
      const float x =
          (code >= 0) ? ((s_codes[player * CONTRIB_BLOCK + tid] == (short)code) ? 1.0f : 0.0f)
                      : s_nums[(player - N_CAT) * CONTRIB_BLOCK + tid];
      const bool right = !(x <= __int_as_float(rec.y));
      o = o && (right == (bool)(rec.w & SHAP_DIR_RIGHT));
      z *= (double)__int_as_float(rec.z);
      const bool last = (r + 1 == r1) || (splits[r + 1].w & SHAP_FIRST);
      if (last) {  // block-uniform
        const double d = (o ? 1.0 : 0.0) - z;
#pragma unroll
        for (int q = 0; q < SHAP_NQ; ++q) L[q] *= fma(d, T[q], z);
        omask |= (o ? 1u : 0u) << m;
        if (tid == 0) sz[m] = z;
        ++m;
        z = 1.0;
        o = true;
      }
    }

    __syncthreads();  // sz complete; previous path's s_rcp reads are done
    for (int j = tid; j < m * SHAP_NQ; j += CONTRIB_BLOCK) {
      const double zp = sz[j / SHAP_NQ];
      s_rcp[j] = 1.0 / fma(1.0 - zp, s_t[j % SHAP_NQ], zp);  // >= t_q > 0
    }
    __syncthreads();

    // pass 2: credit every player of the path
    const double v = (double)leaf_value[leaf];
    double s0 = 0.0;
#pragma unroll
    for (int q = 0; q < SHAP_NQ; ++q) {
      s0 = fma(W[q] / (1.0 - T[q]), L[q], s0);
      L[q] *= W[q];
    }
    int p = 0;
    for (int r = r0; r < r1; ++r) {
      const int w = splits[r].w;
      if (!(w & SHAP_FIRST)) continue;  // block-uniform
      const int player = (w >> SHAP_PLAYER_SHIFT) & 0xFF;
      const double zp = sz[p];
      double phi;
      if ((omask >> p) & 1u) {
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < SHAP_NQ; ++q) s = fma(L[q], s_rcp[p * SHAP_NQ + q], s);
        phi = v * (1.0 - zp) * s;  // exactly 0 when z_p == 1
      } else {
        phi = (zp == 0.0) ? 0.0 : -v * s0;
      }
      s_acc[player * CONTRIB_BLOCK + tid] += phi;
      ++p;
    }
  }

  if (!live) return;
  double* out = shap + (size_t)row * N_SRC;
#pragma unroll
  for (int c = 0; c < N_SRC; ++c) {
    const double a = s_acc[c * CONTRIB_BLOCK + tid];
    if (a != 0.0) atomicAdd(&out[c], a * scale);
  }
}

// Interventional Shapley values against a background sample, over the same
// path table (frac is not read). The game for explained row x and background
// row r: a coalition's hybrid row takes x on its columns and r elsewhere;
// values are averaged over r. Closed form per (x, r, leaf) with leaf value v:
// a_p / b_p = 1 iff x / r satisfies every split of player group p of the
// path. The pair can reach the leaf only if a_p | b_p for every p. Then with
// X = a & ~b, R = ~a & b, nx = |X|, nr = |R|:
//   each i in X gets +v (nx-1)! nr! / (nx+nr)!,
//   each i in R gets -v (nr-1)! nx! / (nx+nr)!,
// and players with a_p & b_p are dummies of the pair. With the masks as
// <= 23-bit words the pair step is one compare, two popcounts and two reads
// of ISHAP_W[a][b] = (a-1)! b! / (a+b)!.
//
// forest_shap_kernel's skeleton: one thread per explained row, CONTRIB_BLOCK
// rows staged column-major in LDS with fused imputation, N_SRC f64
// accumulators per thread in LDS, blockIdx.y strides over paths, all loops
// with block-uniform trip counts (threads past n_rows stay in the barriers
// on a clamped row and only skip the flush). Per path:
//   1. every thread walks the records for its own row -> a; the walk also
//      yields the group -> player map (thread 0 writes it to LDS);
//   2. the block walks the records for the background rows, thread j taking
//      rows j, j + CONTRIB_BLOCK, ... (row-major reads of arrays of at most
//      76 KB that stay in L2, imputation fused) -> one u32 mask per
//      background row in LDS; nothing per (path, background row) goes to HBM;
//   3. barrier; every thread loops over the LDS masks (broadcast reads),
//      skips dead pairs and credits the set bits of X and R;
//   4. barrier (the masks and the map are rewritten by the next path).
// The records are walked (rows + background) x depth per path, not per pair.
// LDS: 33,024 B as forest_contrib_kernel + 4,096 B masks + 4,608 B weight
// table + 92 B group -> player map = 41,820 B static (three blocks per CU).
#define ISHAP_MAX_BACKGROUND 1024
static_assert(N_SRC < 32, "player-group masks are 32-bit words");

// ISHAP_W[a][b] = (a-1)! b! / (a+b)!, a >= 1, from W[a][0] = 1/a and
// W[a][b] = W[a][b-1] * b / (a+b): ratios only, no factorial is formed
// (23! is not exact in f64). cpu_ref.ishap_weight_table does the same.
struct IshapWeights {
  double w[N_SRC + 1][N_SRC + 1];
  constexpr IshapWeights() : w{} {
    for (int a = 1; a <= N_SRC; ++a) {
      w[a][0] = 1.0 / (double)a;
      for (int b = 1; b <= N_SRC; ++b)
        w[a][b] = w[a][b - 1] * (double)b / (double)(a + b);
    }
  }
};
__constant__ IshapWeights ISHAP_W = IshapWeights();

__global__ __launch_bounds__(CONTRIB_BLOCK) void forest_ishap_kernel(
    const short* __restrict__ codes,       // [B, N_CAT]
    const float* __restrict__ nums,        // [B, N_NUM]
    const short* __restrict__ bg_codes,    // [R, N_CAT]
    const float* __restrict__ bg_nums,     // [R, N_NUM], NaNs not yet imputed
    const float* __restrict__ medians,     // [N_NUM]
    const float* __restrict__ leaf_value,  // [L]
    const int* __restrict__ leaf_off,      // [L+1] into splits
    const int4* __restrict__ splits,       // [S] {feat, thr bits, frac bits, flags}
    int n_leaves,
    int n_rows,
    int n_bg,                              // 1 <= R <= ISHAP_MAX_BACKGROUND (host)
    double scale_over_r,                   // (1/T or 1) / R
    double* __restrict__ phi)              // [B, N_SRC], pre-zeroed
{
  __shared__ double s_acc[N_SRC * CONTRIB_BLOCK];
  __shared__ short s_codes[N_CAT * CONTRIB_BLOCK];
  __shared__ float s_nums[N_NUM * CONTRIB_BLOCK];
  __shared__ unsigned s_mask[ISHAP_MAX_BACKGROUND];
  __shared__ double s_w[(N_SRC + 1) * (N_SRC + 1)];
  __shared__ int s_player[N_SRC];  // player of each group of the current path

  const int tid = threadIdx.x;
  const int row_raw = blockIdx.x * CONTRIB_BLOCK + tid;
  const bool live = row_raw < n_rows;
  const int row = live ? row_raw : n_rows - 1;  // n_rows >= 1 (host)

#pragma unroll
  for (int c = 0; c < N_CAT; ++c)
    s_codes[c * CONTRIB_BLOCK + tid] = codes[(size_t)row * N_CAT + c];
#pragma unroll
  for (int c = 0; c < N_NUM; ++c) {
    const float v = nums[(size_t)row * N_NUM + c];
    s_nums[c * CONTRIB_BLOCK + tid] = isnan(v) ? medians[c] : v;
  }
#pragma unroll
  for (int c = 0; c < N_SRC; ++c) s_acc[c * CONTRIB_BLOCK + tid] = 0.0;
  for (int j = tid; j < (N_SRC + 1) * (N_SRC + 1); j += CONTRIB_BLOCK)
    s_w[j] = ISHAP_W.w[j / (N_SRC + 1)][j % (N_SRC + 1)];
  // the first barrier of the path loop orders s_w before its first read; a
  // block whose paths are all skipped never reads it

  for (int leaf = blockIdx.y; leaf < n_leaves; leaf += gridDim.y) {
    const int r0 = leaf_off[leaf];
    const int r1 = leaf_off[leaf + 1];
    if (r1 == r0) continue;  // root leaf: no players (block-uniform)

    // 1. the own row's mask, the group count and the group -> player map
    unsigned a = 0;
    int m = 0;  // player groups closed so far
    bool o = true;
    for (int r = r0; r < r1; ++r) {
      const int4 rec = splits[r];
      const int player = (rec.w >> SHAP_PLAYER_SHIFT) & 0xFF;
      const int code = (int)((unsigned)rec.w >> SHAP_CODE_SHIFT) - 1;
      const float x =
          (code >= 0) ? ((s_codes[player * CONTRIB_BLOCK + tid] == (short)code) ? 1.0f : 0.0f)
                      : s_nums[(player - N_CAT) * CONTRIB_BLOCK + tid];
      const bool right = !(x <= __int_as_float(rec.y));
      o = o && (right == (bool)(rec.w & SHAP_DIR_RIGHT));
      const bool last = (r + 1 == r1) || (splits[r + 1].w & SHAP_FIRST);
      if (last) {  // block-uniform
        if (m < N_SRC) {
          a |= (o ? 1u : 0u) << m;
          if (tid == 0) s_player[m] = player;
        }
        ++m;
        o = true;
      }
    }
    // The host has checked the table (at most N_SRC groups per path); a
    // path that breaks that is skipped, never indexed (block-uniform, and
    // before this iteration's barriers).
    if (m > N_SRC) continue;
    const unsigned full = (1u << m) - 1u;

    // 2. one mask per background row
    for (int k = tid; k < n_bg; k += CONTRIB_BLOCK) {
      const short* bc = bg_codes + (size_t)k * N_CAT;
      const float* bn = bg_nums + (size_t)k * N_NUM;
      unsigned b = 0;
      int g = 0;
      bool ob = true;
      for (int r = r0; r < r1; ++r) {
        const int4 rec = splits[r];
        const int player = (rec.w >> SHAP_PLAYER_SHIFT) & 0xFF;
        const int code = (int)((unsigned)rec.w >> SHAP_CODE_SHIFT) - 1;
        float x;
        if (code >= 0) {
          x = (bc[player] == (short)code) ? 1.0f : 0.0f;
        } else {
          x = bn[player - N_CAT];
          if (isnan(x)) x = medians[player - N_CAT];
        }
        const bool right = !(x <= __int_as_float(rec.y));
        ob = ob && (right == (bool)(rec.w & SHAP_DIR_RIGHT));
        const bool last = (r + 1 == r1) || (splits[r + 1].w & SHAP_FIRST);
        if (last) {
          b |= (ob ? 1u : 0u) << g;
          ++g;
          ob = true;
        }
      }
      s_mask[k] = b;
    }
    __syncthreads();  // masks, s_player (and s_w on the first path) complete

    // 3. the pairs of this thread's row
    const double v = (double)leaf_value[leaf];
    for (int k = 0; k < n_bg; ++k) {
      const unsigned b = s_mask[k];
      if ((a | b) != full) continue;  // no coalition reaches the leaf
      unsigned mx = a & ~b;
      unsigned mr = b & ~a;
      if ((mx | mr) == 0u) continue;  // every player a dummy of the pair
      const int nx = __popc(mx);
      const int nr = __popc(mr);
      const double wp = v * s_w[nx * (N_SRC + 1) + nr];
      const double wn = v * s_w[nr * (N_SRC + 1) + nx];
      while (mx) {
        const int g = __ffs((int)mx) - 1;
        mx &= mx - 1u;
        s_acc[s_player[g] * CONTRIB_BLOCK + tid] += wp;
      }
      while (mr) {
        const int g = __ffs((int)mr) - 1;
        mr &= mr - 1u;
        s_acc[s_player[g] * CONTRIB_BLOCK + tid] -= wn;
      }
    }
    __syncthreads();  // the next path rewrites s_mask and s_player
  }

  if (!live) return;
  double* out = phi + (size_t)row * N_SRC;
#pragma unroll
  for (int c = 0; c < N_SRC; ++c) {
    const double acc = s_acc[c * CONTRIB_BLOCK + tid];
    if (acc != 0.0) atomicAdd(&out[c], acc * scale_over_r);
  }
}

// Exact path-dependent SHAP interaction values over the same path table.
// For one leaf with value v and distinct players p on its path (z_p, o_p as
// in forest_shap_kernel), the Shapley interaction index of i != j is
//
//   Phi_ij = v/2 (o_i - z_i)(o_j - z_j) int_0^1 prod_{p != i,j} f_p(t) dt,
//   f_p(t) = z_p (1-t) + o_p t
//
// (degree <= N_SRC - 2, the SHAP_NQ-point rule is exact). With f_pq, L_q as
// above and g_pq = (o_p - z_p) / f_pq:  Phi_ij = v/2 sum_q w_q L_q g_iq g_jq.
//   o_p = 0: g_pq = -1 / (1 - t_q), a constant table (z_p cancels; with
//            z_p = 0, L_q is exactly 0 and so is every pair of the leaf);
//   o_p = 1: g_pq = (1 - z_p) / f_pq depends on the path only and is computed
//            once per path into LDS; exactly 0 when z_p = 1.
// No 0/0 can form: f_pq >= t_q > 0 wherever a quotient is taken.
//
// A row needs 253 f64 accumulators (unordered player pairs), so the split is
// not forest_shap_kernel's: a block stages SHAPI_ROWS = 16 rows column-major
// with fused imputation and SHAPI_TPR = 16 threads serve each row
// (tid = k * SHAPI_ROWS + row, so a wavefront holds all 16 rows x 4 values
// of k and the rows of one k hit 16 consecutive doubles). Per path:
//   1. every thread walks the records for its row -> o-mask; thread k <
//      SHAP_NQ also carries the one product L_k and writes w_k L_k to LDS;
//      the thread of row r keeps z of groups r and r + 16 and writes their
//      g_pk afterwards (one or two divisions per thread, not one per group
//      per wavefront); thread 0 writes the group -> player map;
//   2. barrier; every thread takes the 12 w_q L_q of its row into registers
//      and the m(m-1)/2 group pairs are dealt round-robin over k. The pair a
//      thread handles in an iteration is block-uniform (s_pair decodes it),
//      only the o-cases differ by row. Two groups of a path are different
//      players and a pair has one owner k, so no two threads touch the same
//      accumulator within a path;
//   3. barrier (the next path rewrites the tables and may hand an
//      accumulator to another thread of the row).
// Both barriers sit in the path loop, whose trip count and skips (root leaf,
// more than N_SRC groups: skipped, never indexed) are block-uniform; threads
// past n_rows work on a clamped row and only skip the flush. The flush is
// one atomicAdd per non-zero (row, pair) per block into the upper triangle;
// the binding mirrors it (both sides bit-equal) and the diagonal is the
// caller's (engine: phi_i minus the off-diagonal row sum).
// LDS: 253*16*8 B accumulators 32,384 + rows 1,184 + w L 1,536 + g 2,208 +
// g-off 96 + map 92 + pair table 506 = 38,006 B static (four blocks per CU).
#define SHAPI_ROWS 16
#define SHAPI_TPR 16
#define SHAPI_BLOCK (SHAPI_ROWS * SHAPI_TPR)
#define SHAPI_PAIRS (N_SRC * (N_SRC - 1) / 2)
static_assert(SHAPI_TPR >= SHAP_NQ, "one thread of a row per quadrature node");
static_assert(2 * SHAPI_ROWS >= N_SRC, "two group slots per row index cover a path");
static_assert(N_SRC <= SHAPI_BLOCK, "the pair table is filled one column per thread");

__global__ __launch_bounds__(SHAPI_BLOCK) void forest_shap_inter_kernel(
    const short* __restrict__ codes,       // [B, N_CAT]
    const float* __restrict__ nums,        // [B, N_NUM]
    const float* __restrict__ medians,     // [N_NUM]
    const float* __restrict__ leaf_value,  // [L]
    const int* __restrict__ leaf_off,      // [L+1] into splits
    const int4* __restrict__ splits,       // [S] {feat, thr bits, frac bits, flags}
    int n_leaves,
    int n_rows,
    double half_scale,                     // (1/T or 1) / 2
    double* __restrict__ inter)            // [B, N_SRC, N_SRC], pre-zeroed; upper triangle
{
  constexpr double T[SHAP_NQ] = {SHAP_T_LIST};
  constexpr double W[SHAP_NQ] = {SHAP_W_LIST};

  __shared__ double s_acc[SHAPI_PAIRS * SHAPI_ROWS];  // [hi(hi-1)/2 + lo][row]
  __shared__ short s_codes[N_CAT * SHAPI_ROWS];
  __shared__ float s_nums[N_NUM * SHAPI_ROWS];
  __shared__ double s_wl[SHAP_NQ * SHAPI_ROWS];       // w_q L_q of each row
  __shared__ double s_g[N_SRC * SHAP_NQ];             // g_pq for o_p = 1
  __shared__ double s_goff[SHAP_NQ];                  // g_pq for o_p = 0
  __shared__ int s_player[N_SRC];                     // player of each group
  __shared__ unsigned short s_pair[SHAPI_PAIRS];      // b(b-1)/2 + a -> a | b << 8

  const int tid = threadIdx.x;
  const int ri = tid % SHAPI_ROWS;
  const int k = tid / SHAPI_ROWS;
  const int row_raw = blockIdx.x * SHAPI_ROWS + ri;
  const bool live = row_raw < n_rows;
  const int row = live ? row_raw : n_rows - 1;  // n_rows >= 1 (host)

  for (int c = k; c < N_CAT; c += SHAPI_TPR)
    s_codes[c * SHAPI_ROWS + ri] = codes[(size_t)row * N_CAT + c];
  for (int c = k; c < N_NUM; c += SHAPI_TPR) {
    const float v = nums[(size_t)row * N_NUM + c];
    s_nums[c * SHAPI_ROWS + ri] = isnan(v) ? medians[c] : v;
  }
  for (int j = tid; j < SHAPI_PAIRS * SHAPI_ROWS; j += SHAPI_BLOCK) s_acc[j] = 0.0;
  if (tid >= 1 && tid < N_SRC)
    for (int a = 0; a < tid; ++a)
      s_pair[tid * (tid - 1) / 2 + a] = (unsigned short)(a | (tid << 8));
  double tk = 0.0, wk = 0.0;  // this thread's quadrature node
#pragma unroll
  for (int q = 0; q < SHAP_NQ; ++q)
    if (k == q) {
      tk = T[q];
      wk = W[q];
      if (ri == 0) s_goff[q] = -1.0 / (1.0 - T[q]);
    }
  __syncthreads();  // the staged rows are read across k

  for (int leaf = blockIdx.y; leaf < n_leaves; leaf += gridDim.y) {
    const int r0 = leaf_off[leaf];
    const int r1 = leaf_off[leaf + 1];
    if (r1 == r0) continue;  // root leaf: no players (block-uniform)

    // pass 1: o-mask of the row, L_k, and z of the groups this thread owns
    unsigned omask = 0;
    int m = 0;  // player groups closed so far
    double z = 1.0, lk = 1.0, z0 = 1.0, z1 = 1.0;
    bool o = true;
    for (int r = r0; r < r1; ++r) {
      const int4 rec = splits[r];
      const int player = (rec.w >> SHAP_PLAYER_SHIFT) & 0xFF;
      const int code = (int)((unsigned)rec.w >> SHAP_CODE_SHIFT) - 1;
      const float x =
          (code >= 0) ? ((s_codes[player * SHAPI_ROWS + ri] == (short)code) ? 1.0f : 0.0f)
                      : s_nums[(player - N_CAT) * SHAPI_ROWS + ri];
      const bool right = !(x <= __int_as_float(rec.y));
      o = o && (right == (bool)(rec.w & SHAP_DIR_RIGHT));
      z *= (double)__int_as_float(rec.z);
      const bool last = (r + 1 == r1) || (splits[r + 1].w & SHAP_FIRST);
      if (last) {  // block-uniform
        if (m < N_SRC) {
          lk *= fma((o ? 1.0 : 0.0) - z, tk, z);
          omask |= (o ? 1u : 0u) << m;
          if (m == ri) z0 = z;
          if (m == ri + SHAPI_ROWS) z1 = z;
          if (tid == 0) s_player[m] = player;
        }
        ++m;
        z = 1.0;
        o = true;
      }
    }
    // The host has checked the table (at most N_SRC groups per path); a
    // path that breaks that is skipped, never indexed (block-uniform, and
    // before this iteration's barriers).
    if (m > N_SRC) continue;
    if (k < SHAP_NQ) {
      s_wl[k * SHAPI_ROWS + ri] = wk * lk;
      if (ri < m)
        s_g[ri * SHAP_NQ + k] = (1.0 - z0) / fma(1.0 - z0, tk, z0);  // f >= t_k > 0
      if (ri + SHAPI_ROWS < m)
        s_g[(ri + SHAPI_ROWS) * SHAP_NQ + k] = (1.0 - z1) / fma(1.0 - z1, tk, z1);
    }
    __syncthreads();  // s_wl, s_g, s_player complete

    // pass 2: this thread's share of the path's group pairs
    double wl[SHAP_NQ];
#pragma unroll
    for (int q = 0; q < SHAP_NQ; ++q) wl[q] = s_wl[q * SHAPI_ROWS + ri];
    const double v = (double)leaf_value[leaf];
    const int n_pairs = m * (m - 1) / 2;
    for (int pr = k; pr < n_pairs; pr += SHAPI_TPR) {
      const int ab = s_pair[pr];
      const int a = ab & 0xFF;
      const int b = ab >> 8;
      const double* ga = ((omask >> a) & 1u) ? &s_g[a * SHAP_NQ] : s_goff;
      const double* gb = ((omask >> b) & 1u) ? &s_g[b * SHAP_NQ] : s_goff;
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < SHAP_NQ; ++q) s = fma(wl[q] * ga[q], gb[q], s);
      const int pa = s_player[a];
      const int pb = s_player[b];
      const int lo = min(pa, pb);
      const int hi = max(pa, pb);
      if (lo != hi)  // always, by the table's construction; keeps the index in range
        s_acc[(hi * (hi - 1) / 2 + lo) * SHAPI_ROWS + ri] += v * s;
    }
    __syncthreads();  // the next path rewrites the tables
  }

  if (!live) return;
  double* out = inter + (size_t)row * N_SRC * N_SRC;
  for (int pr = k; pr < SHAPI_PAIRS; pr += SHAPI_TPR) {
    const double acc = s_acc[pr * SHAPI_ROWS + ri];
    if (acc != 0.0) {
      const int ab = s_pair[pr];
      atomicAdd(&out[(ab & 0xFF) * N_SRC + (ab >> 8)], acc * half_scale);
    }
  }
}

// What-if forest sums for partial dependence / ICE curves: the raw classifier
// sum (leaf payloads over ALL trees, as forest_kernel<false> accumulates them)
// of every sample row under every job's overrides. A job {player0, bits0,
// player1, bits1} replaces one or two source columns of the row: player is
// the schema feature index of the attribution kernels (0..N_CAT-1 the
// categorical columns, N_CAT..N_SRC-1 the numerics, -1 = no override, slot 1
// only); bits is the category code, or the f32 bit pattern of the value. An
// overridden numeric takes the job's value even where the row holds NaN; an
// overridden categorical answers every one-hot test of its column.
//
// One thread per row, one WAVE per block (WHATIF_BLOCK = 64): rows staged
// column-major in LDS with fused imputation exactly as forest_kernel, 74 B per
// row, each thread touching only its own slots, so no barrier anywhere.
// blockIdx.y strides over the jobs; per job the thread saves its own one or
// two slots, writes the override, walks every tree and restores. One thread
// owns all trees of a (job, row): the result is a plain store, deterministic,
// no atomics, no pre-zeroed output. The walk keeps WHATIF_ILP consecutive
// trees in flight (independent gather chains hide the node latency) and adds
// their leaves afterwards in tree order, so the f64 sum is the tree-order sum
// whatever the interleaving. Work per launch is jobs x rows threads; the
// default call (256 rows, a few hundred jobs) is ~1600 one-wave blocks, which
// spread over the 1024 SIMDs far more evenly than 400 four-wave blocks.
#define WHATIF_BLOCK 64
#define WHATIF_ILP 4

__global__ __launch_bounds__(WHATIF_BLOCK) void forest_whatif_kernel(
    const short* __restrict__ codes,    // [R, N_CAT]
    const float* __restrict__ nums,     // [R, N_NUM], NaNs not yet imputed
    const float* __restrict__ medians,  // [N_NUM]
    const int4* __restrict__ nodes,     // [n_nodes] {feat, bits, left, right}
    const int* __restrict__ tree_off,   // [T+1]
    int n_trees,
    const int* __restrict__ feat_col,   // [F]
    const int* __restrict__ feat_code,  // [F]
    const int4* __restrict__ jobs,      // [J] {player0, bits0, player1, bits1}
    int n_jobs,
    int n_rows,
    double* __restrict__ out)           // [J, R]; every entry is written
{
  __shared__ short s_codes[N_CAT * WHATIF_BLOCK];
  __shared__ float s_nums[N_NUM * WHATIF_BLOCK];

  const int tid = threadIdx.x;
  const int row = blockIdx.x * WHATIF_BLOCK + tid;
  if (row >= n_rows) return;  // no barrier below: own LDS slots only

#pragma unroll
  for (int c = 0; c < N_CAT; ++c)
    s_codes[c * WHATIF_BLOCK + tid] = codes[(size_t)row * N_CAT + c];
#pragma unroll
  for (int c = 0; c < N_NUM; ++c) {
    const float v = nums[(size_t)row * N_NUM + c];
    s_nums[c * WHATIF_BLOCK + tid] = isnan(v) ? medians[c] : v;
  }

  // Writes the override of one job slot into the thread's own LDS column and
  // returns what stood there (as bits), for the restore. The host has checked
  // the players; the unsigned compare also drops slot 1's -1.
  auto swap_in = [&](int player, int bits) -> int {
    int old = 0;
    if ((unsigned)player < (unsigned)N_CAT) {
      old = s_codes[player * WHATIF_BLOCK + tid];
      s_codes[player * WHATIF_BLOCK + tid] = (short)bits;
    } else if ((unsigned)player < (unsigned)N_SRC) {
      old = __float_as_int(s_nums[(player - N_CAT) * WHATIF_BLOCK + tid]);
      s_nums[(player - N_CAT) * WHATIF_BLOCK + tid] = __int_as_float(bits);
    }
    return old;
  };

  for (int j = blockIdx.y; j < n_jobs; j += gridDim.y) {
    const int4 job = jobs[j];
    const int old0 = swap_in(job.x, job.y);
    const int old1 = swap_in(job.z, job.w);

    double local = 0.0;
    for (int t = 0; t < n_trees; t += WHATIF_ILP) {
      int4 nd[WHATIF_ILP];
      int base[WHATIF_ILP];
#pragma unroll
      for (int k = 0; k < WHATIF_ILP; ++k) {
        base[k] = 0;
        nd[k] = make_int4(-1, 0, 0, 0);  // past the last tree: a leaf of +0.0
        if (t + k < n_trees) {
          base[k] = tree_off[t + k];
          nd[k] = nodes[base[k]];
        }
      }
      bool any = true;
      while (any) {
        any = false;
#pragma unroll
        for (int k = 0; k < WHATIF_ILP; ++k) {
          if (nd[k].x >= 0) {
            const int col = feat_col[nd[k].x];
            const int code = feat_code[nd[k].x];
            const float v =
                (code >= 0) ? ((s_codes[col * WHATIF_BLOCK + tid] == (short)code) ? 1.0f : 0.0f)
                            : s_nums[col * WHATIF_BLOCK + tid];
            nd[k] = nodes[base[k] + ((v <= __int_as_float(nd[k].y)) ? nd[k].z : nd[k].w)];
            any = true;
          }
        }
      }
#pragma unroll
      for (int k = 0; k < WHATIF_ILP; ++k) local += (double)__int_as_float(nd[k].y);
    }
    out[(size_t)j * n_rows + row] = local;

    // restore in reverse order (the host refuses player0 == player1 anyway)
    swap_in(job.z, old1);
    swap_in(job.x, old0);
  }
}

// Accumulated local effects (ALE): per (row, entry) the raw classifier sum of
// the row with ONE numeric column set to the lower and to the upper edge of the
// grid interval the row's own value lies in. An entry is {numeric player, its
// ascending f32 edges z[0..Ke]}; interval k = clip(#{z < x}, 1, Ke) is
// (z[k-1], z[k]], found by the thread itself with f32 compares (a binary
// search over the entry's edges, staged in LDS once per block and entry; the
// host sends no per-row table). Outputs: interval[e, row] = k and
// sums[e, row] = {S at z[k-1], S at z[k]}, each the tree-order f64 sum that
// forest_whatif_kernel gives for that value, bit for bit.
//
// Work split as forest_whatif_kernel: one thread owns a (row, entry) pair and
// all of its trees, one wave per block, rows staged column-major in LDS with
// fused imputation (own slots only), blockIdx.y strides over the entries. The
// only shared LDS is the edge list, hence the two barriers per entry; they
// are why no thread leaves early (threads past the last row idle along).
//
// Dual walk. The two walks of a pair differ only at nodes on the swept column
// whose threshold lies in [lo, hi), so a tree is walked with ONE cursor for
// as long as both values take the same branch: a node on another column or a
// one-hot node is decided once by the row, a node on the swept column is
// decided for lo and for hi. If lo <= thr < hi the walk forks: cursor A goes
// on with lo, cursor B with hi, and each decides every later node itself (it
// may meet the swept column again). Cursors of one tree never meet again, so
// "forked" is one bit per tree. ALE_ILP trees are in flight per thread (up
// to 2 x ALE_ILP independent gather chains once forked); both leaves of each
// are added to the two sums afterwards, in tree order.
//
// Bounds by construction (the note on forest_sweep_kernel): a tree whose
// [base, base + size) does not lie inside the node table is skipped, a node
// index is compared unsigned against the tree's node count before every load
// (a bad one ends the cursor on a leaf of +0.0), a feature index outside the
// table reads as a leaf, source columns are clamped, the walk loop runs at
// most size times, and the interval search is bounded by its halving range.
#define ALE_BLOCK 64
#define ALE_ILP 4
#define ALE_MAX_EDGES 128

// Generated without packed f32 VALU instructions, per function (as the MMD
// kernels are), so that every other kernel of this file keeps its code.
#if defined(__HIP_DEVICE_COMPILE__)
#define ALE_NO_PACKED_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define ALE_NO_PACKED_F32
#endif

// Whether the cursor on split node `nd` goes left for the thread's staged row
// with `swept_v` standing in the swept numeric column `col` (one-hot test or
// numeric column, clamped); `on_swept` tells whether the node tests `col`.
__device__ __forceinline__ bool ale_goes_left(
    int4 nd, const int* __restrict__ feat_col, const int* __restrict__ feat_code,
    const short* s_codes, const float* s_nums, int tid, int col, float swept_v,
    bool& on_swept)
{
  const int fcol = feat_col[nd.x];
  const int code = feat_code[nd.x];
  on_swept = code < 0 && fcol == col;
  const float v = (code >= 0)
      ? ((s_codes[min((unsigned)fcol, (unsigned)(N_CAT - 1)) * ALE_BLOCK + tid] == (short)code)
             ? 1.0f : 0.0f)
      : (on_swept ? swept_v
                  : s_nums[min((unsigned)fcol, (unsigned)(N_NUM - 1)) * ALE_BLOCK + tid]);
  return v <= __int_as_float(nd.y);
}

// Node `rel` of the tree at `base` with `size` nodes; an index outside the
// tree reads as a leaf of +0.0 and is never used to index.
__device__ __forceinline__ int4 ale_load(
    const int4* __restrict__ nodes, int base, unsigned size, int rel)
{
  return ((unsigned)rel < size) ? nodes[base + rel] : make_int4(-1, 0, 0, 0);
}

ALE_NO_PACKED_F32 __global__ __launch_bounds__(ALE_BLOCK) void forest_ale_kernel(
    const short* __restrict__ codes,    // [R, N_CAT]
    const float* __restrict__ nums,     // [R, N_NUM], NaNs not yet imputed
    const float* __restrict__ medians,  // [N_NUM]
    const int4* __restrict__ nodes,     // [n_nodes] {feat, bits, left, right}
    const int* __restrict__ tree_off,   // [T+1]
    int n_trees,
    unsigned n_nodes,
    const int* __restrict__ feat_col,   // [F]
    const int* __restrict__ feat_code,  // [F]
    unsigned n_feat,
    const int* __restrict__ players,    // [E] numeric schema indices
    const int* __restrict__ edge_off,   // [E+1]
    const float* __restrict__ edges,    // ragged, ascending per entry
    int n_entries,
    int n_rows,
    int* __restrict__ interval,         // [E, R]; every entry is written
    double2* __restrict__ sums)         // [E, R] {S(lo), S(hi)}; all written
{
  __shared__ short s_codes[N_CAT * ALE_BLOCK];
  __shared__ float s_nums[N_NUM * ALE_BLOCK];
  __shared__ float s_edges[ALE_MAX_EDGES];

  const int tid = threadIdx.x;
  const int row = blockIdx.x * ALE_BLOCK + tid;
  const bool live = row < n_rows;

  if (live) {
#pragma unroll
    for (int c = 0; c < N_CAT; ++c)
      s_codes[c * ALE_BLOCK + tid] = codes[(size_t)row * N_CAT + c];
#pragma unroll
    for (int c = 0; c < N_NUM; ++c) {
      const float v = nums[(size_t)row * N_NUM + c];
      s_nums[c * ALE_BLOCK + tid] = isnan(v) ? medians[c] : v;
    }
  }

  const int4 dead = make_int4(-1, 0, 0, 0);  // a leaf of +0.0

  for (int e = blockIdx.y; e < n_entries; e += gridDim.y) {
    // block-uniform: the entry's column and edges
    const int e0 = edge_off[e];
    const int n_edge = min(max(edge_off[e + 1] - e0, 0), ALE_MAX_EDGES);
    const int col = (int)min((unsigned)(players[e] - N_CAT), (unsigned)(N_NUM - 1));
    __syncthreads();  // the entry before is done with s_edges
    for (int i = tid; i < n_edge; i += ALE_BLOCK) s_edges[i] = edges[e0 + i];
    __syncthreads();
    if (!live || n_edge < 2) continue;  // the host refuses n_edge < 2

    // k = clip(#{z < x}, 1, Ke): the first edge that is not below x
    const float x = s_nums[col * ALE_BLOCK + tid];
    int first = 0, last = n_edge;
    while (first < last) {
      const int mid = (first + last) >> 1;
      if (s_edges[mid] < x) first = mid + 1; else last = mid;
    }
    const int k = min(max(first, 1), n_edge - 1);
    const float lo = s_edges[k - 1];
    const float hi = s_edges[k];

    double sum_lo = 0.0, sum_hi = 0.0;
    for (int t = 0; t < n_trees; t += ALE_ILP) {
      int4 a[ALE_ILP], b[ALE_ILP];
      int base[ALE_ILP];
      unsigned size[ALE_ILP];
      bool forked[ALE_ILP];
      unsigned longest = 0;
#pragma unroll
      for (int s = 0; s < ALE_ILP; ++s) {
        base[s] = 0;
        size[s] = 0;
        forked[s] = false;
        a[s] = dead;
        b[s] = dead;
        if (t + s < n_trees) {
          const int b0 = tree_off[t + s];
          const int sz = tree_off[t + s + 1] - b0;
          if (b0 >= 0 && sz > 0 && (unsigned)b0 + (unsigned)sz <= n_nodes) {
            base[s] = b0;
            size[s] = (unsigned)sz;
            a[s] = nodes[b0];
          }
        }
        longest = max(longest, size[s]);
      }
      bool any = true;
      for (unsigned it = 0; it < longest && any; ++it) {
        any = false;
#pragma unroll
        for (int s = 0; s < ALE_ILP; ++s) {
          // cursor B first: a fork made below takes its first own step in
          // the next round, after both loads have been issued
          if (forked[s] && (unsigned)b[s].x < n_feat) {
            bool on_swept;
            const bool left = ale_goes_left(b[s], feat_col, feat_code, s_codes, s_nums, tid,
                                            col, hi, on_swept);
            b[s] = ale_load(nodes, base[s], size[s], left ? b[s].z : b[s].w);
            any = true;
          }
          if ((unsigned)a[s].x < n_feat) {
            bool on_swept;
            const bool left = ale_goes_left(a[s], feat_col, feat_code, s_codes, s_nums, tid,
                                            col, lo, on_swept);
            if (!forked[s] && on_swept && left && !(hi <= __int_as_float(a[s].y))) {
              forked[s] = true;  // lo <= thr < hi: hi goes right
              b[s] = ale_load(nodes, base[s], size[s], a[s].w);
            }
            a[s] = ale_load(nodes, base[s], size[s], left ? a[s].z : a[s].w);
            any = true;
          }
        }
      }
      // a cursor the loop bound stopped on a split (bad tables only) adds 0
#pragma unroll
      for (int s = 0; s < ALE_ILP; ++s) {
        if (t + s < n_trees) {
          const int4 fin = forked[s] ? b[s] : a[s];
          sum_lo += ((unsigned)a[s].x < n_feat) ? 0.0 : (double)__int_as_float(a[s].y);
          sum_hi += ((unsigned)fin.x < n_feat) ? 0.0 : (double)__int_as_float(fin.y);
        }
      }
    }
    const size_t at = (size_t)e * n_rows + row;
    interval[at] = k;
    sums[at] = make_double2(sum_lo, sum_hi);
  }
}

// Permutation importance: out[q, row] is the raw classifier sum of the row
// with ONE source column replaced by the value another row (the donor
// perm[q, row]) holds there. Table row q permutes schema player
// perm_player[q] (0..N_CAT-1 a categorical column, N_CAT..N_SRC-1 a numeric).
// A numeric donor gives its imputed value (NaN -> the median); a categorical
// donor's code answers every one-hot test of the column. Each entry is the
// tree-order f64 sum forest_whatif_kernel gives for that one override, bit for
// bit; unlike a what-if job the override differs from row to row.
//
// Work split as forest_whatif_kernel: one thread owns a (job, row) and all
// trees, one wave per block, rows staged column-major in LDS with fused
// imputation (own slots only, so no barrier), blockIdx.y strides over the
// jobs, plain stores. A job {player, q0, n} is up to PERM_ILP consecutive
// table rows of one player (the repeats of a feature; the launcher groups
// them). The thread reads its n donor values into registers and never writes
// the LDS slot, so there is nothing to restore.
//
// Shared base walk. The n walks of a tree are identical down to the first
// node that tests the job's column, so the thread walks the row's own values
// ONCE to that node (or to the leaf if the path never tests the column: then
// all n sums take that leaf and the tree has cost one walk, not n). From that
// node n cursors go on side by side, the ILP slots that WHATIF_ILP spends on
// trees; each decides every later node itself, with its donor value at nodes
// of the job's column (it may be tested again further down) and the row's LDS
// value elsewhere. Leaves are added per tree, so every sum is in tree order.
//
// Bounds by construction (the note on forest_ale_kernel): a tree outside the
// node table is skipped, a node index is compared unsigned against the tree's
// size before every load, a feature index outside the table reads as a leaf,
// base walk and cursors together take at most `size` steps, source columns,
// table rows and donor indices are clamped.
#define PERM_BLOCK 64
#define PERM_ILP 4

// The staged row's own value at split node `nd` (one-hot test or numeric
// column, clamped); `code` is the node's category code (-1: numeric) and
// `on_player` tells whether the node tests the job's column.
__device__ __forceinline__ float perm_own_value(
    int4 nd, const int* __restrict__ feat_col, const int* __restrict__ feat_code,
    const short* s_codes, const float* s_nums, int tid, bool cat_job, int pcol,
    int& code, bool& on_player)
{
  const int fcol = feat_col[nd.x];
  code = feat_code[nd.x];
  on_player = ((code >= 0) == cat_job) && fcol == pcol;
  return (code >= 0)
      ? ((s_codes[min((unsigned)fcol, (unsigned)(N_CAT - 1)) * PERM_BLOCK + tid] == (short)code)
             ? 1.0f : 0.0f)
      : s_nums[min((unsigned)fcol, (unsigned)(N_NUM - 1)) * PERM_BLOCK + tid];
}

ALE_NO_PACKED_F32 __global__ __launch_bounds__(PERM_BLOCK) void forest_permute_kernel(
    const short* __restrict__ codes,    // [R, N_CAT]
    const float* __restrict__ nums,     // [R, N_NUM], NaNs not yet imputed
    const float* __restrict__ medians,  // [N_NUM]
    const int4* __restrict__ nodes,     // [n_nodes] {feat, bits, left, right}
    const int* __restrict__ tree_off,   // [T+1]
    int n_trees,
    unsigned n_nodes,
    const int* __restrict__ feat_col,   // [F]
    const int* __restrict__ feat_code,  // [F]
    unsigned n_feat,
    const int4* __restrict__ jobs,      // [J] {player, q0, n, 0}
    int n_jobs,
    const int* __restrict__ perm,       // [Q, R] donor rows
    int n_q,
    int n_rows,
    double* __restrict__ out)           // [Q, R]; every entry is written
{
  __shared__ short s_codes[N_CAT * PERM_BLOCK];
  __shared__ float s_nums[N_NUM * PERM_BLOCK];

  const int tid = threadIdx.x;
  const int row = blockIdx.x * PERM_BLOCK + tid;
  if (row >= n_rows) return;  // no barrier below: own LDS slots only

#pragma unroll
  for (int c = 0; c < N_CAT; ++c)
    s_codes[c * PERM_BLOCK + tid] = codes[(size_t)row * N_CAT + c];
#pragma unroll
  for (int c = 0; c < N_NUM; ++c) {
    const float v = nums[(size_t)row * N_NUM + c];
    s_nums[c * PERM_BLOCK + tid] = isnan(v) ? medians[c] : v;
  }

  const int4 dead = make_int4(-1, 0, 0, 0);  // a leaf of +0.0

  for (int j = blockIdx.y; j < n_jobs; j += gridDim.y) {
    const int4 job = jobs[j];
    const bool cat_job = (unsigned)job.x < (unsigned)N_CAT;
    const int pcol = cat_job ? job.x
                             : (int)min((unsigned)(job.x - N_CAT), (unsigned)(N_NUM - 1));
    const int q0 = min(max(job.y, 0), n_q - 1);
    const int n = min(max(job.z, 0), min(PERM_ILP, n_q - q0));

    // the donors' values in the job's column: a category code, or the bits
    // of the imputed f32
    int donor_bits[PERM_ILP];
#pragma unroll
    for (int i = 0; i < PERM_ILP; ++i) {
      donor_bits[i] = 0;
      if (i < n) {
        const size_t d = min((unsigned)perm[(size_t)(q0 + i) * n_rows + row],
                             (unsigned)(n_rows - 1));
        if (cat_job) {
          donor_bits[i] = codes[d * N_CAT + pcol];
        } else {
          const float v = nums[d * N_NUM + pcol];
          donor_bits[i] = __float_as_int(isnan(v) ? medians[pcol] : v);
        }
      }
    }

    double sum[PERM_ILP];
#pragma unroll
    for (int i = 0; i < PERM_ILP; ++i) sum[i] = 0.0;

    for (int t = 0; t < n_trees; ++t) {
      const int b0 = tree_off[t];
      const int sz = tree_off[t + 1] - b0;
      if (b0 < 0 || sz <= 0 || (unsigned)b0 + (unsigned)sz > n_nodes) continue;
      const unsigned size = (unsigned)sz;

      // the shared base walk, on the row's own values
      int4 cur = nodes[b0];
      bool resume = false;
      unsigned it = 0;
      for (; it < size && (unsigned)cur.x < n_feat; ++it) {
        int code;
        const float v = perm_own_value(cur, feat_col, feat_code, s_codes, s_nums, tid,
                                       cat_job, pcol, code, resume);
        if (resume) break;
        cur = ale_load(nodes, b0, size, (v <= __int_as_float(cur.y)) ? cur.z : cur.w);
      }

      if (!resume) {
        // the path never tests the column: one leaf for all repeats (a walk
        // the loop bound stopped on a split, bad tables only, adds 0)
        const double leaf = ((unsigned)cur.x < n_feat) ? 0.0 : (double)__int_as_float(cur.y);
#pragma unroll
        for (int i = 0; i < PERM_ILP; ++i) sum[i] += leaf;  // slots past n are not stored
        continue;
      }

      // n cursors from the first node on the job's column
      int4 c[PERM_ILP];
#pragma unroll
      for (int i = 0; i < PERM_ILP; ++i) c[i] = (i < n) ? cur : dead;
      bool any = true;
      for (; it < size && any; ++it) {
        any = false;
#pragma unroll
        for (int i = 0; i < PERM_ILP; ++i) {
          if ((unsigned)c[i].x < n_feat) {
            int code;
            bool on_player;
            float v = perm_own_value(c[i], feat_col, feat_code, s_codes, s_nums, tid,
                                     cat_job, pcol, code, on_player);
            if (on_player)
              v = cat_job ? (((short)donor_bits[i] == (short)code) ? 1.0f : 0.0f)
                          : __int_as_float(donor_bits[i]);
            c[i] = ale_load(nodes, b0, size, (v <= __int_as_float(c[i].y)) ? c[i].z : c[i].w);
            any = true;
          }
        }
      }
#pragma unroll
      for (int i = 0; i < PERM_ILP; ++i)
        sum[i] += ((unsigned)c[i].x < n_feat) ? 0.0 : (double)__int_as_float(c[i].y);
    }

#pragma unroll
    for (int i = 0; i < PERM_ILP; ++i)
      if (i < n) out[(size_t)(q0 + i) * n_rows + row] = sum[i];
  }
}

// Anchor rules: per candidate anchor of a row, the number of background sample
// rows whose COMPOSITE has a raw classifier sum above `cut`. An anchor is a
// u32 set of schema players (the numbering of forest_whatif_kernel). The
// composite z(i, A, b) of row i, anchor A and sample row b is the sample row
// with every player of A & ~sat[i, b] replaced by row i's own (imputed)
// value; sat[i, b] is the host's set of players whose predicate, taken from
// row i, sample row b satisfies already (creditcore/anchors.py), and those
// keep the sample's value. Row i's candidates are masks[mask_off[i] ..
// mask_off[i + 1]); the host cuts them into jobs {row, first mask, n} of at
// most ANCHOR_CHUNK = 64 masks.
//
// Work split: one-wave blocks, blockIdx.x the job, blockIdx.y striding over
// the 64-row passes of the sample; thread `tid` owns sample row b0 + tid of a
// pass and ALL trees, for all masks of the job at once. Row i (imputed), the pass's sample rows (column-major,
// imputed, own slots only) and has[p], the u64 set of the job's masks that
// contain player p, are staged in LDS; the thread's sat word is a register.
//
// Shared walk. All masks of a job see the same tree and differ only in which
// players they replace, so a tree is walked once with cursors (node, live),
// live a u64 set of the job's masks, all of them at the root. At a node on
// player p the branch is taken under row i's value (gx) and under the sample
// row's (gb). If p is in sat, or gx == gb, every composite goes gb. Otherwise
// live & has[p] goes gx and live & ~has[p] goes gb; an empty side is not
// walked, and of two live sides one is pushed on the thread's stack. After a
// split live is uniform in p, so a path splits at most once per player and
// the stack never holds more than N_SRC entries of 12 B (LDS, own slots).
// At a leaf its value is added, as f64, to the accumulator of every mask in
// live (64 f64 per thread in LDS, own slots). The leaves of a tree partition
// the masks, so every accumulator takes exactly one add per tree, tree after
// tree: the sum is the tree-order sum of walking the composite row on its
// own, bit for bit (forest_whatif_kernel wherever a composite is at most two
// overrides). One tree is in flight per thread; that keeps the order trivially.
//
// Counts: after the last tree each accumulator is compared with `cut`, the
// wave's votes are counted with one ballot per mask, and lane m keeps mask
// m's count over the block's passes: a plain store at the end into the
// block's own row of counts[gridDim.y, M] (the launcher adds the rows: counts
// are integers), no atomics, no pre-zeroed output. `sums` (tests, the
// micro-benchmark) may be null.
//
// Bounds by construction (the note on forest_sweep_kernel): a tree outside
// the node table is skipped, a node index is compared unsigned against the
// tree's size before every load, a feature index outside the table reads as a
// leaf, players and the job's row and mask range are clamped, the walk of a
// tree takes at most `size` steps over all of its cursors, and a push checks
// the stack's N_SRC slots (a full stack, bad tables only, drops that side).
#define ANCHOR_BLOCK 64
#define ANCHOR_CHUNK 64
#define ANCHOR_STACK N_SRC

__global__ __launch_bounds__(ANCHOR_BLOCK) void forest_anchor_kernel(
    const short* __restrict__ codes,     // [R, N_CAT] the rows to explain
    const float* __restrict__ nums,      // [R, N_NUM], NaNs not yet imputed
    const short* __restrict__ bg_codes,  // [S, N_CAT] the sample
    const float* __restrict__ bg_nums,   // [S, N_NUM], NaNs not yet imputed
    const float* __restrict__ medians,   // [N_NUM]
    const int4* __restrict__ nodes,      // [n_nodes] {feat, bits, left, right}
    const int* __restrict__ tree_off,    // [T+1]
    int n_trees,
    unsigned n_nodes,
    const int* __restrict__ feat_col,    // [F]
    const int* __restrict__ feat_code,   // [F]
    unsigned n_feat,
    const unsigned* __restrict__ sat,    // [R, S]
    const unsigned* __restrict__ masks,  // [M]
    const int4* __restrict__ jobs,       // [J] {row, first mask, n, 0}
    int n_rows,
    int n_bg,
    int n_masks,                         // M >= 1
    double cut,
    int* __restrict__ counts,            // [gridDim.y, M]; every entry is written
    double* __restrict__ sums)           // [M, S] or null; all written
{
  typedef unsigned long long u64;
  __shared__ double s_acc[ANCHOR_CHUNK * ANCHOR_BLOCK];
  __shared__ u64 s_stk_live[ANCHOR_STACK * ANCHOR_BLOCK];
  __shared__ int s_stk_node[ANCHOR_STACK * ANCHOR_BLOCK];
  __shared__ u64 s_has[N_SRC];
  __shared__ short s_codes[N_CAT * ANCHOR_BLOCK];
  __shared__ float s_nums[N_NUM * ANCHOR_BLOCK];
  __shared__ short s_xc[N_CAT];
  __shared__ float s_xn[N_NUM];

  const int tid = threadIdx.x;
  const int4 job = jobs[blockIdx.x];
  const int row = min(max(job.x, 0), n_rows - 1);
  const int m0 = min(max(job.y, 0), n_masks - 1);
  const int nm = min(max(job.z, 0), min(ANCHOR_CHUNK, n_masks - m0));

  // block-uniform tables: row i, imputed, and the chunk's per-player sets
  if (tid < N_CAT) {
    s_xc[tid] = codes[(size_t)row * N_CAT + tid];
  } else if (tid < N_SRC) {
    const float v = nums[(size_t)row * N_NUM + (tid - N_CAT)];
    s_xn[tid - N_CAT] = isnan(v) ? medians[tid - N_CAT] : v;
  }
  if (tid < N_SRC) {
    u64 h = 0;
    for (int k = 0; k < nm; ++k) h |= (u64)((masks[m0 + k] >> tid) & 1u) << k;
    s_has[tid] = h;
  }
  __syncthreads();

  const u64 all = (nm >= 64) ? ~0ull : ((1ull << nm) - 1ull);
  int my_count = 0;  // lane m: mask m0 + m

  for (int b0 = blockIdx.y * ANCHOR_BLOCK; b0 < n_bg; b0 += gridDim.y * ANCHOR_BLOCK) {
    const int b = b0 + tid;
    const bool active = b < n_bg;  // idle lanes still vote below
    if (active) {
#pragma unroll
      for (int c = 0; c < N_CAT; ++c)
        s_codes[c * ANCHOR_BLOCK + tid] = bg_codes[(size_t)b * N_CAT + c];
#pragma unroll
      for (int c = 0; c < N_NUM; ++c) {
        const float v = bg_nums[(size_t)b * N_NUM + c];
        s_nums[c * ANCHOR_BLOCK + tid] = isnan(v) ? medians[c] : v;
      }
      const unsigned sat_w = sat[(size_t)row * n_bg + b];
      for (int m = 0; m < nm; ++m) s_acc[m * ANCHOR_BLOCK + tid] = 0.0;

      for (int t = 0; t < n_trees; ++t) {
        const int base = tree_off[t];
        const int sz = tree_off[t + 1] - base;
        if (base < 0 || sz <= 0 || (unsigned)base + (unsigned)sz > n_nodes) continue;
        const unsigned size = (unsigned)sz;

        int4 nd = nodes[base];
        u64 live = all;
        int sp = 0;
        for (unsigned it = 0; it < size; ++it) {
          if ((unsigned)nd.x >= n_feat) {  // a leaf: one add per live mask
            const double v = (double)__int_as_float(nd.y);
            for (u64 l = live; l != 0ull; l &= l - 1ull)
              s_acc[(__ffsll((long long)l) - 1) * ANCHOR_BLOCK + tid] += v;
            if (sp == 0) break;
            --sp;
            live = s_stk_live[sp * ANCHOR_BLOCK + tid];
            nd = ale_load(nodes, base, size, s_stk_node[sp * ANCHOR_BLOCK + tid]);
            continue;
          }
          const int fcol = feat_col[nd.x];
          const int code = feat_code[nd.x];
          int p;
          float vx, vb;
          if (code >= 0) {
            p = (int)min((unsigned)fcol, (unsigned)(N_CAT - 1));
            vx = (s_xc[p] == (short)code) ? 1.0f : 0.0f;
            vb = (s_codes[p * ANCHOR_BLOCK + tid] == (short)code) ? 1.0f : 0.0f;
          } else {
            const int c = (int)min((unsigned)fcol, (unsigned)(N_NUM - 1));
            p = N_CAT + c;
            vx = s_xn[c];
            vb = s_nums[c * ANCHOR_BLOCK + tid];
          }
          const float thr = __int_as_float(nd.y);
          const bool gx = vx <= thr;
          const bool gb = vb <= thr;
          int next = gb ? nd.z : nd.w;
          if (gx != gb && !((sat_w >> p) & 1u)) {
            const u64 has = s_has[p];
            const u64 lx = live & has;
            const u64 lb = live & ~has;
            if (lx != 0ull) {
              if (lb != 0ull && sp < ANCHOR_STACK) {
                s_stk_live[sp * ANCHOR_BLOCK + tid] = lb;
                s_stk_node[sp * ANCHOR_BLOCK + tid] = next;
                ++sp;
              }
              live = lx;
              next = gx ? nd.z : nd.w;
            }
          }
          nd = ale_load(nodes, base, size, next);
        }
      }

      if (sums != nullptr)
        for (int m = 0; m < nm; ++m)
          sums[(size_t)(m0 + m) * n_bg + b] = s_acc[m * ANCHOR_BLOCK + tid];
    }

    // nm and b0 are block-uniform: every lane of the wave reaches each ballot
    for (int m = 0; m < nm; ++m) {
      const bool over = active && s_acc[m * ANCHOR_BLOCK + tid] > cut;
      const int c = __popcll(__ballot(over));
      if (tid == m) my_count += c;
    }
  }
  if (tid < nm) counts[(size_t)blockIdx.y * n_masks + m0 + tid] = my_count;
}

// Exact single-feature sweep for counterfactuals: the raw classifier sum of
// one row as ONE numeric column moves over the whole real line, every other
// column held fixed. The sum is piecewise constant in that column; its
// breakpoints are the K distinct f32 thresholds the forest tests on it
// (creditcore/counterfactual.py builds them, sorted, with the rank of every
// node's threshold in node_rank). Interval k is (T[k-1], T[k]], K+1 in all.
//
// A job is {row, numeric column}. A tree is walked ONCE per job and chunk of
// the curve, depth first, left child first, carrying the rank range [lo, hi)
// that reaches the node: a node on another column (or a one-hot node) is
// decided by the row, a node of rank r on the swept column sends
// [lo, min(hi, r+1)) left and [max(lo, r+1), hi) right, and an empty half is
// not descended. Left first means the leaves come out in ascending rank order
// and tile the range, so a tree's answer is a short list {end, leaf}: segment
// s covers [end[s-1], end[s]). The stack holds {right child, hi} of the nodes
// whose both halves are alive; the range's lo is the end of the last segment.
//
// One block of SWEEP_BLOCK threads per (job, chunk of SWEEP_CHUNK intervals).
// Phase A: thread u walks tree b0+u (a batch of SWEEP_BLOCK trees) restricted
// to the chunk's range and leaves its segment list in LDS (SWEEP_SEG_CAP
// segments; a path tests one column only a few times). Phase B: every thread
// owns SWEEP_IPT consecutive intervals in registers and goes through the
// batch IN TREE ORDER, adding the leaf of the segment each interval falls
// in (broadcast LDS reads). A tree with more segments than the list holds is
// re-walked in phase B by each thread over its own few intervals: slower,
// still exact, still in tree order. So every interval's f64 sum is the
// tree-order sum forest_whatif_kernel computes for a value inside it: plain
// stores, no atomics, bit-identical to the reference.
//
// Bounds by construction: node indices are compared unsigned against the
// tree's node count before every load, the walk loop runs at most that many
// times (a depth-first walk sees a node once), the stack push is guarded by
// SWEEP_MAX_DEPTH (the host refuses deeper forests before any launch),
// source columns are clamped and curve stores are guarded by the chunk's end.
#define SWEEP_BLOCK 256
#define SWEEP_IPT 4
#define SWEEP_CHUNK (SWEEP_BLOCK * SWEEP_IPT)
#define SWEEP_SEG_CAP 8
#define SWEEP_MAX_DEPTH 64

template <class Emit>
__device__ __forceinline__ void sweep_walk_tree(
    const int4* __restrict__ nodes, const int* __restrict__ node_rank,
    int base, unsigned n_tree_nodes,
    const int* __restrict__ feat_col, const int* __restrict__ feat_code, unsigned n_feat,
    const short* s_codes, const float* s_nums,
    int col, int lo, int hi, Emit&& emit)
{
  int stk_node[SWEEP_MAX_DEPTH];
  int stk_hi[SWEEP_MAX_DEPTH];
  int sp = 0;
  unsigned rel = 0;
  for (unsigned it = 0; it < n_tree_nodes; ++it) {
    if (rel >= n_tree_nodes) return;
    const int4 nd = nodes[base + rel];
    if ((unsigned)nd.x >= n_feat) {  // a leaf (feat = -1)
      emit(hi, __int_as_float(nd.y));
      if (sp == 0) return;
      --sp;
      lo = hi;
      rel = (unsigned)stk_node[sp];
      hi = stk_hi[sp];
      continue;
    }
    const int fcol = feat_col[nd.x];
    const int code = feat_code[nd.x];
    if (code < 0 && fcol == col) {
      const int mid = node_rank[base + rel] + 1;  // ranks <= r go left
      if (mid >= hi) {
        rel = (unsigned)nd.z;
      } else if (mid <= lo) {
        rel = (unsigned)nd.w;
      } else {
        if ((unsigned)sp < (unsigned)SWEEP_MAX_DEPTH) {
          stk_node[sp] = nd.w;
          stk_hi[sp] = hi;
          ++sp;
        }
        hi = mid;
        rel = (unsigned)nd.z;
      }
    } else {
      const float v =
          (code >= 0) ? ((s_codes[min((unsigned)fcol, (unsigned)(N_CAT - 1))] == (short)code) ? 1.0f : 0.0f)
                      : s_nums[min((unsigned)fcol, (unsigned)(N_NUM - 1))];
      rel = (unsigned)((v <= __int_as_float(nd.y)) ? nd.z : nd.w);
    }
  }
}

__global__ __launch_bounds__(SWEEP_BLOCK) void forest_sweep_kernel(
    const short* __restrict__ codes,     // [R, N_CAT]
    const float* __restrict__ nums,      // [R, N_NUM], NaNs not yet imputed
    const float* __restrict__ medians,   // [N_NUM]
    const int4* __restrict__ nodes,      // [n_nodes] {feat, bits, left, right}
    const int* __restrict__ node_rank,   // [n_nodes] threshold rank, -1 = none
    const int* __restrict__ tree_off,    // [T+1]
    int n_trees,
    unsigned n_nodes,
    const int* __restrict__ feat_col,    // [F]
    const int* __restrict__ feat_code,   // [F]
    unsigned n_feat,
    const int* __restrict__ thr_off,     // [N_NUM+1] offsets of the threshold lists
    const int2* __restrict__ jobs,       // [J] {row, numeric column}
    const long long* __restrict__ curve_off,  // [J] first curve entry of the job
    int n_jobs,
    int n_rows,
    double* __restrict__ curves)         // ragged: K+1 sums per job, all written
{
  __shared__ short s_codes[N_CAT];
  __shared__ float s_nums[N_NUM];
  __shared__ int s_end[SWEEP_SEG_CAP * SWEEP_BLOCK];
  __shared__ float s_val[SWEEP_SEG_CAP * SWEEP_BLOCK];
  __shared__ int s_nseg[SWEEP_BLOCK];

  const int tid = threadIdx.x;
  const int j = blockIdx.x;
  if (j >= n_jobs) return;
  const int2 job = jobs[j];
  const int row = job.x, col = job.y;
  if ((unsigned)row >= (unsigned)n_rows || (unsigned)col >= (unsigned)N_NUM) return;
  const int n_int = thr_off[col + 1] - thr_off[col] + 1;  // K + 1 intervals
  const long long c0l = (long long)blockIdx.y * SWEEP_CHUNK;
  if (c0l >= n_int) return;  // the grid is sized for the longest curve
  const int c0 = (int)c0l;
  const int c1 = min(c0 + SWEEP_CHUNK, n_int);

  // the job's row, imputed exactly as forest_whatif_kernel stages its rows
  if (tid < N_CAT) s_codes[tid] = codes[(size_t)row * N_CAT + tid];
  if (tid >= 32 && tid < 32 + N_NUM) {
    const float v = nums[(size_t)row * N_NUM + (tid - 32)];
    s_nums[tid - 32] = isnan(v) ? medians[tid - 32] : v;
  }
  __syncthreads();

  const int kb = c0 + tid * SWEEP_IPT;  // the thread's own intervals
  double acc[SWEEP_IPT];
#pragma unroll
  for (int i = 0; i < SWEEP_IPT; ++i) acc[i] = 0.0;

  for (int b0 = 0; b0 < n_trees; b0 += SWEEP_BLOCK) {
    // phase A: one tree per thread, its segment list into LDS
    const int t = b0 + tid;
    if (t < n_trees) {
      const int base = tree_off[t];
      const int size = tree_off[t + 1] - base;
      int n = 0;
      if (base >= 0 && size > 0 && (unsigned)base + (unsigned)size <= n_nodes) {
        sweep_walk_tree(nodes, node_rank, base, (unsigned)size, feat_col, feat_code, n_feat,
                        s_codes, s_nums, col, c0, c1, [&](int end, float v) {
                          if (n < SWEEP_SEG_CAP) {
                            s_end[n * SWEEP_BLOCK + tid] = end;
                            s_val[n * SWEEP_BLOCK + tid] = v;
                          }
                          ++n;
                        });
      }
      s_nseg[tid] = min(n, SWEEP_SEG_CAP + 1);
    }
    __syncthreads();

    // phase B: the batch in tree order
    const int nb = min(SWEEP_BLOCK, n_trees - b0);
    for (int u = 0; u < nb; ++u) {
      const int n = s_nseg[u];
      if (n == 1) {  // the tree does not see the column on this row's path
        const double v = (double)s_val[u];
#pragma unroll
        for (int i = 0; i < SWEEP_IPT; ++i) acc[i] += v;
      } else if (n <= SWEEP_SEG_CAP) {
        if (n > 0) {
#pragma unroll
          for (int i = 0; i < SWEEP_IPT; ++i) {
            int s = 0;
            while (s + 1 < n && kb + i >= s_end[s * SWEEP_BLOCK + u]) ++s;
            acc[i] += (double)s_val[s * SWEEP_BLOCK + u];
          }
        }
      } else if (kb < c1) {  // list overflow: walk the tree over the own intervals
        const int base = tree_off[b0 + u];
        const int size = tree_off[b0 + u + 1] - base;  // checked in phase A (n > 0)
        int cur = kb;
        sweep_walk_tree(nodes, node_rank, base, (unsigned)size, feat_col, feat_code, n_feat,
                        s_codes, s_nums, col, kb, min(kb + SWEEP_IPT, c1),
                        [&](int end, float v) {
#pragma unroll
                          for (int i = 0; i < SWEEP_IPT; ++i)
                            if (kb + i >= cur && kb + i < end) acc[i] += (double)v;
                          cur = end;
                        });
      }
    }
    __syncthreads();  // the lists are rewritten by the next batch
  }

  double* out = curves + curve_off[j];
#pragma unroll
  for (int i = 0; i < SWEEP_IPT; ++i)
    if (kb + i < c1) out[kb + i] = acc[i];
}

// Search phase of the sweep: per job the row's own interval k0 (the number of
// thresholds below its imputed value) and the nearest interval on each side
// whose decision `raw > cut` differs from the decision at k0. One block per
// job strides over the curve; the two nearest indices are reduced with
// integer LDS atomics (order-free). Record {k0, k_below, k_above}, -1 = none,
// and the three raw sums (0.0 where there is none).
__global__ __launch_bounds__(SWEEP_BLOCK) void forest_sweep_search_kernel(
    const float* __restrict__ nums,      // [R, N_NUM]
    const float* __restrict__ medians,   // [N_NUM]
    const float* __restrict__ thr,       // thresholds of all columns, sorted per column
    const int* __restrict__ thr_off,     // [N_NUM+1]
    const int2* __restrict__ jobs,       // [J]
    const long long* __restrict__ curve_off,  // [J]
    const double* __restrict__ curves,
    double cut,
    int n_jobs,
    int n_rows,
    int* __restrict__ rec,               // [J, 3]
    double* __restrict__ raw)            // [J, 3]
{
  __shared__ int s_below, s_above;
  const int tid = threadIdx.x;
  const int j = blockIdx.x;
  if (j >= n_jobs) return;
  const int2 job = jobs[j];
  const int row = job.x, col = job.y;
  if ((unsigned)row >= (unsigned)n_rows || (unsigned)col >= (unsigned)N_NUM) return;
  const int t0 = thr_off[col];
  const int K = thr_off[col + 1] - t0;
  float v = nums[(size_t)row * N_NUM + col];
  if (isnan(v)) v = medians[col];
  int a = 0, b = K;  // lower bound: the number of thresholds < v
  while (a < b) {
    const int m = (a + b) >> 1;
    if (thr[t0 + m] < v) a = m + 1; else b = m;
  }
  const int k0 = a;  // 0..K
  const double* c = curves + curve_off[j];
  const bool d0 = c[k0] > cut;
  if (tid == 0) { s_below = -1; s_above = K + 1; }
  __syncthreads();
  int below = -1, above = K + 1;
  for (int k = tid; k <= K; k += SWEEP_BLOCK) {
    if ((c[k] > cut) != d0) {
      if (k < k0) below = max(below, k);
      else above = min(above, k);  // k != k0: the decision at k0 is d0
    }
  }
  if (below >= 0) atomicMax(&s_below, below);
  if (above <= K) atomicMin(&s_above, above);
  __syncthreads();
  if (tid == 0) {
    const int kb = s_below, ka = (s_above <= K) ? s_above : -1;
    rec[3 * j] = k0;
    rec[3 * j + 1] = kb;
    rec[3 * j + 2] = ka;
    raw[3 * j] = c[k0];
    raw[3 * j + 1] = (kb >= 0) ? c[kb] : 0.0;
    raw[3 * j + 2] = (ka >= 0) ? c[ka] : 0.0;
  }
}

// 4-tree ILP + optional transposed grid (blockIdx.x = tree chunk so the
// dispatcher's id%8 XCD placement gives adjacent chunks to different XCDs,
// keeping each XCD's L2 on a tree subset). Experimental A/B variants.
template <bool DIRECT, int ILP, bool SWAP_GRID>
__global__ __launch_bounds__(BLOCK) void forest_kernel_ilpN(
    const short* __restrict__ codes,
    const float* __restrict__ nums,
    const float* __restrict__ medians,
    const int4* __restrict__ nodes,
    const int* __restrict__ tree_off,
    int n_trees,
    const int* __restrict__ feat_col,
    const int* __restrict__ feat_code,
    int n_rows,
    double* __restrict__ acc)
{
  __shared__ short s_codes[N_CAT * BLOCK];
  __shared__ float s_nums[N_NUM * BLOCK];
  const int tid = threadIdx.x;
  const int row_blk = SWAP_GRID ? blockIdx.y : blockIdx.x;
  const int chunk = SWAP_GRID ? blockIdx.x : blockIdx.y;
  const int n_chunks = SWAP_GRID ? gridDim.x : gridDim.y;
  const int row = row_blk * BLOCK + tid;
  if (row < n_rows) {
    if (!DIRECT) {
#pragma unroll
      for (int c = 0; c < N_CAT; ++c) s_codes[c * BLOCK + tid] = codes[row * N_CAT + c];
    }
#pragma unroll
    for (int c = 0; c < N_NUM; ++c) {
      const float v = nums[row * N_NUM + c];
      s_nums[c * BLOCK + tid] = isnan(v) ? medians[c] : v;
    }
  }
  if (row >= n_rows) return;

  auto value_of = [&](int f) -> float {
    if (DIRECT) return s_nums[f * BLOCK + tid];
    const int col = feat_col[f];
    const int code = feat_code[f];
    return (code >= 0) ? ((s_codes[col * BLOCK + tid] == (short)code) ? 1.0f : 0.0f)
                       : s_nums[col * BLOCK + tid];
  };

  double local = 0.0;
  for (int t = chunk; t < n_trees; t += ILP * n_chunks) {
    int4 nd[ILP];
    int base[ILP];
    bool live[ILP];
#pragma unroll
    for (int k = 0; k < ILP; ++k) {
      const int tk = t + k * n_chunks;
      live[k] = tk < n_trees;
      if (live[k]) {
        base[k] = tree_off[tk];
        nd[k] = nodes[base[k]];
      }
    }
    bool any = true;
    while (any) {
      any = false;
#pragma unroll
      for (int k = 0; k < ILP; ++k) {
        if (!live[k]) continue;
        if (nd[k].x >= 0) {
          const float v = value_of(nd[k].x);
          nd[k] = nodes[base[k] + ((v <= __int_as_float(nd[k].y)) ? nd[k].z : nd[k].w)];
          any = true;
        } else {
          local += (double)__int_as_float(nd[k].y);
          live[k] = false;
        }
      }
    }
  }
  atomicAdd(&acc[row], local);
}

__global__ __launch_bounds__(BLOCK) void finalize_kernel(
    double* __restrict__ cls_acc,
    double* __restrict__ if_acc,
    int n_rows,
    int cls_kind,        // 0 = RF leaf-fraction mean; 1 = GBT logit sum
    double inv_n_trees,
    double cls_bias,
    double if_denom,
    double if_offset,
    double if_threshold,
    double* __restrict__ proba,
    double* __restrict__ iscore,
    double* __restrict__ outlier)
{
  const int i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n_rows) return;
  proba[i] = cls_kind ? 1.0 / (1.0 + exp(-(cls_acc[i] + cls_bias)))
                      : cls_acc[i] * inv_n_trees;
  // alibi instance_score = -(sklearn decision_function)
  //                      = 2^(-mean_depth_sum/denom) + offset_
  const double anomaly = exp2(-if_acc[i] / if_denom);
  const double s = anomaly + if_offset;
  iscore[i] = s;
  outlier[i] = (s > if_threshold) ? 1.0 : 0.0;
  // zero-after-read: the accumulators start all-zero (torch::zeros at
  // session init) and every finalize re-zeros the rows it consumed, so no
  // per-request memset node is needed in the graph regardless of how batch
  // sizes interleave across captured shapes
  cls_acc[i] = 0.0;
  if_acc[i] = 0.0;
}

// ---------------------------------------------------------------------------
// Drift statistics
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(BLOCK) void cat_hist_kernel(
    const short* __restrict__ codes,  // [B, N_CAT]
    int n_rows,
    const int* __restrict__ cat_off,  // [N_CAT+1]
    int total_bins,
    int* __restrict__ hist)           // [total_bins], pre-zeroed
{
  extern __shared__ int s_hist[];
  for (int i = threadIdx.x; i < total_bins; i += blockDim.x) s_hist[i] = 0;
  __syncthreads();
  __shared__ int s_off[N_CAT + 1];
  if (threadIdx.x <= N_CAT) s_off[threadIdx.x] = cat_off[threadIdx.x];
  __syncthreads();

  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n_rows;
       r += gridDim.x * blockDim.x) {
#pragma unroll
    for (int c = 0; c < N_CAT; ++c) {
      const int lo = s_off[c];
      const int nbins = s_off[c + 1] - lo;
      const int code = codes[r * N_CAT + c];
      // unknown/unseen category (-1) lands in the trailing "unseen" bin,
      // matching creditcore.ops.cpu_ref.drift_stats_cpu
      const int bin = (code < 0) ? (nbins - 1) : code;
      atomicAdd(&s_hist[lo + bin], 1);
    }
  }
  __syncthreads();
  if (gridDim.x == 1) {
    // single-block launch (small batches): plain stores — the output needs
    // no pre-zero memset node in the graph
    for (int i = threadIdx.x; i < total_bins; i += blockDim.x)
      hist[i] = s_hist[i];
  } else {
    for (int i = threadIdx.x; i < total_bins; i += blockDim.x)
      if (s_hist[i] != 0) atomicAdd(&hist[i], s_hist[i]);
  }
}

// One block per numeric feature. Sorts the (imputed) batch column in LDS with
// a bitonic sort, then evaluates sup|F_ref - F_batch| at every batch point's
// left/right limits (the extrema of two step CDFs — same algorithm as
// creditcore.models.drift.ks_2samp_d). CDF arithmetic in f64 to match the
// CPU reference bitwise-closely. When the reference column fits the
// remaining LDS (160 KiB/CU on gfx950) it is staged there too, so the
// per-element binary searches hit LDS instead of bouncing off L2.
template <int BS>
__global__ __launch_bounds__(BS) void ks_kernel_t(
    const float* __restrict__ nums,       // [B, n_cols]
    const float* __restrict__ medians,    // [n_cols]
    int n_cols,                           // feature count == gridDim.x
    int n_rows,
    int m_pow2,                           // next pow2 >= n_rows
    int ref_lds,                          // 1 => stage ref column in LDS
    const float* __restrict__ ref_sorted, // concatenated per-feature refs
    const int64_t* __restrict__ rs_off,   // [n_cols+1] (i64: offsets exceed
                                          // 2^31 for HBM-scale references)
    float* __restrict__ ks_d)             // [n_cols]
{
  extern __shared__ float s_vals[];  // [m_pow2] batch | [n_ref] staged ref
  const int j = blockIdx.x;
  const int m = n_rows;

  for (int i = threadIdx.x; i < m_pow2; i += blockDim.x) {
    float v = INFINITY;
    if (i < m) {
      v = nums[i * n_cols + j];
      if (isnan(v)) v = medians[j];
    }
    s_vals[i] = v;
  }
  const int64_t ref_lo = rs_off[j];
  const int n_ref_j = (int)(rs_off[j + 1] - ref_lo);
  if (ref_lds) {
    float* s_ref = s_vals + m_pow2;
    for (int i = threadIdx.x; i < n_ref_j; i += blockDim.x)
      s_ref[i] = ref_sorted[ref_lo + i];
  }
  __syncthreads();

  // bitonic sort (ascending)
  for (int k = 2; k <= m_pow2; k <<= 1) {
    for (int s = k >> 1; s > 0; s >>= 1) {
      for (int i = threadIdx.x; i < m_pow2; i += blockDim.x) {
        const int p = i ^ s;
        if (p > i) {
          const float a = s_vals[i];
          const float b = s_vals[p];
          const bool up = ((i & k) == 0);
          if ((a > b) == up) {
            s_vals[i] = b;
            s_vals[p] = a;
          }
        }
      }
      __syncthreads();
    }
  }

  const int n = n_ref_j;
  const float* __restrict__ ref = ref_lds ? (s_vals + m_pow2) : (ref_sorted + ref_lo);

  double dmax = 0.0;
  for (int i = threadIdx.x; i < m; i += blockDim.x) {
    const float b = s_vals[i];
    int l = 0, r = n;  // lower_bound in ref
    while (l < r) {
      const int mid = (l + r) >> 1;
      if (ref[mid] < b) l = mid + 1; else r = mid;
    }
    const int sl = l;
    r = n;  // upper_bound in ref (resume from sl)
    while (l < r) {
      const int mid = (l + r) >> 1;
      if (ref[mid] <= b) l = mid + 1; else r = mid;
    }
    const int sr = l;
    // F_batch one-sided limits at b: the tie run's bounds in the sorted
    // batch, not the per-element rank (matches models/drift.ks_2samp_d).
    int bl = 0;
    r = i;  // lower_bound of b within s_vals[0..i]
    while (bl < r) {
      const int mid = (bl + r) >> 1;
      if (s_vals[mid] < b) bl = mid + 1; else r = mid;
    }
    int br = i + 1;
    r = m;  // upper_bound of b within s_vals[i+1..m)
    while (br < r) {
      const int mid = (br + r) >> 1;
      if (s_vals[mid] <= b) br = mid + 1; else r = mid;
    }
    const double fl = fabs((double)sl / n - (double)bl / m);
    const double fr = fabs((double)sr / n - (double)br / m);
    dmax = fmax(dmax, fmax(fl, fr));
  }

  // wave reduce (64-wide) then cross-wave via LDS (reuse s_vals after sync)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    dmax = fmax(dmax, __shfl_down(dmax, off, 64));
  __syncthreads();
  float* s_red = s_vals;  // one slot per wave
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) s_red[wave] = (float)dmax;
  __syncthreads();
  if (threadIdx.x == 0) {
    float d = s_red[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) d = fmaxf(d, s_red[w]);
    ks_d[j] = d;
  }
}

// Small-batch K-S variant: instead of a bitonic sort (log^2(B)/2 barriered
// LDS passes — 55 stages at B=1024, ~39 us with only n_cols workgroups on
// the chip), count each element's strict / non-strict rank directly with an
// O(B^2) LDS sweep. The inner loop reads s_vals[k] at the same k across the
// whole wavefront (LDS broadcast, no bank conflicts, no barriers), so at
// B<=2048 the quadratic sweep is several times faster than the sort's
// barrier chain. Output is bitwise-identical to ks_kernel_t: lt/le ARE the
// sorted path's tie-run lower/upper bounds, and the ref binary searches and
// f64 CDF arithmetic are the same (models/drift.ks_2samp_d semantics).
template <int BS>
__global__ __launch_bounds__(BS) void ks_count_kernel_t(
    const float* __restrict__ nums,       // [B, n_cols]
    const float* __restrict__ medians,    // [n_cols]
    int n_cols, int n_rows,
    const float* __restrict__ ref_sorted, const int64_t* __restrict__ rs_off,
    float* __restrict__ ks_d)
{
  extern __shared__ float s_vals[];  // [n_rows] imputed batch column
  const int j = blockIdx.x;
  const int m = n_rows;
  for (int i = threadIdx.x; i < m; i += blockDim.x) {
    float v = nums[i * n_cols + j];
    if (isnan(v)) v = medians[j];
    s_vals[i] = v;
  }
  const int64_t ref_lo = rs_off[j];
  const int n = (int)(rs_off[j + 1] - ref_lo);
  const float* __restrict__ ref = ref_sorted + ref_lo;
  __syncthreads();

  double dmax = 0.0;
  for (int i = threadIdx.x; i < m; i += blockDim.x) {
    const float x = s_vals[i];
    int lt = 0, le = 0;  // # batch elements < x / <= x
    int k = 0;
    for (; k + 3 < m; k += 4) {
      const float v0 = s_vals[k], v1 = s_vals[k + 1];
      const float v2 = s_vals[k + 2], v3 = s_vals[k + 3];
      lt += (int)(v0 < x) + (int)(v1 < x) + (int)(v2 < x) + (int)(v3 < x);
      le += (int)(v0 <= x) + (int)(v1 <= x) + (int)(v2 <= x) + (int)(v3 <= x);
    }
    for (; k < m; ++k) {
      const float v = s_vals[k];
      lt += (int)(v < x);
      le += (int)(v <= x);
    }
    int l = 0, r = n;  // lower_bound in ref
    while (l < r) {
      const int mid = (l + r) >> 1;
      if (ref[mid] < x) l = mid + 1; else r = mid;
    }
    const int sl = l;
    r = n;  // upper_bound in ref (resume from sl)
    while (l < r) {
      const int mid = (l + r) >> 1;
      if (ref[mid] <= x) l = mid + 1; else r = mid;
    }
    const int sr = l;
    const double fl = fabs((double)sl / n - (double)lt / m);
    const double fr = fabs((double)sr / n - (double)le / m);
    dmax = fmax(dmax, fmax(fl, fr));
  }

#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    dmax = fmax(dmax, __shfl_down(dmax, off, 64));
  __syncthreads();
  float* s_red = s_vals;  // one slot per wave (launch smem floors at BS/64)
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) s_red[wave] = (float)dmax;
  __syncthreads();
  if (threadIdx.x == 0) {
    float d = s_red[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) d = fmaxf(d, s_red[w]);
    ks_d[j] = d;
  }
}

// counting beats the sort only while the quadratic sweep stays tiny:
// measured on MI355X, counting is 51 us at B=1024 vs the bitonic's 38.6 us
// (the LDS-broadcast sweep is ALU-bound, not barrier-bound), but wins
// clearly on the small batches the single-call latency path serves
constexpr int KS_COUNT_MAX_ROWS = 256;

// Multi-block counting K-S: the single-block kernels occupy only n_cols
// (=14) of the 256 CUs. This variant splits each column's element range
// over gridDim.y blocks — every block stages the full imputed column in
// LDS (B ≤ 16384 ⇒ ≤ 64 KiB) and sweeps its slice with the same
// LDS-broadcast quadratic count, so ~200+ workgroups fill the chip and
// the O(B²) work parallelizes. Per-(column, block) partial maxima land in
// `scratch`; ks_count_reduce_kernel folds them into ks_d. lt/le counting
// is identical to the single-block kernels (sorted-path tie-run bounds),
// and f64→f32 casting commutes with max, so the result is bitwise equal
// to ks_kernel_t's.
template <int BS>
__global__ __launch_bounds__(BS) void ks_count_mb_kernel_t(
    const float* __restrict__ nums,       // [B, n_cols]
    const float* __restrict__ medians,    // [n_cols]
    int n_cols, int n_rows,
    const float* __restrict__ ref_sorted, const int64_t* __restrict__ rs_off,
    float* __restrict__ scratch)          // [n_cols, gridDim.y]
{
  extern __shared__ float s_vals[];  // [n_rows] imputed batch column
  const int j = blockIdx.x;
  const int m = n_rows;
  for (int i = threadIdx.x; i < m; i += blockDim.x) {
    float v = nums[i * n_cols + j];
    if (isnan(v)) v = medians[j];
    s_vals[i] = v;
  }
  const int64_t ref_lo = rs_off[j];
  const int n = (int)(rs_off[j + 1] - ref_lo);
  const float* __restrict__ ref = ref_sorted + ref_lo;
  __syncthreads();

  // this block's element slice: [e0, e1)
  const int per = (m + gridDim.y - 1) / gridDim.y;
  const int e0 = blockIdx.y * per;
  const int e1 = min(m, e0 + per);

  double dmax = 0.0;
  for (int i = e0 + threadIdx.x; i < e1; i += blockDim.x) {
    const float x = s_vals[i];
    int lt = 0, le = 0;
    int k = 0;
    for (; k + 3 < m; k += 4) {
      const float v0 = s_vals[k], v1 = s_vals[k + 1];
      const float v2 = s_vals[k + 2], v3 = s_vals[k + 3];
      lt += (int)(v0 < x) + (int)(v1 < x) + (int)(v2 < x) + (int)(v3 < x);
      le += (int)(v0 <= x) + (int)(v1 <= x) + (int)(v2 <= x) + (int)(v3 <= x);
    }
    for (; k < m; ++k) {
      const float v = s_vals[k];
      lt += (int)(v < x);
      le += (int)(v <= x);
    }
    int l = 0, r = n;
    while (l < r) {
      const int mid = (l + r) >> 1;
      if (ref[mid] < x) l = mid + 1; else r = mid;
    }
    const int sl = l;
    r = n;
    while (l < r) {
      const int mid = (l + r) >> 1;
      if (ref[mid] <= x) l = mid + 1; else r = mid;
    }
    const int sr = l;
    const double fl = fabs((double)sl / n - (double)lt / m);
    const double fr = fabs((double)sr / n - (double)le / m);
    dmax = fmax(dmax, fmax(fl, fr));
  }

#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    dmax = fmax(dmax, __shfl_down(dmax, off, 64));
  __syncthreads();
  float* s_red = s_vals;  // one slot per wave (smem floors at BS/64)
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) s_red[wave] = (float)dmax;
  __syncthreads();
  if (threadIdx.x == 0) {
    float d = s_red[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) d = fmaxf(d, s_red[w]);
    scratch[(int64_t)j * gridDim.y + blockIdx.y] = d;
  }
}

__global__ __launch_bounds__(64) void ks_count_reduce_kernel(
    const float* __restrict__ scratch,  // [n_cols, g]
    int g, int n_cols,
    float* __restrict__ ks_d)
{
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= n_cols) return;
  float d = 0.0f;
  for (int k = 0; k < g; ++k) d = fmaxf(d, scratch[(int64_t)j * g + k]);
  ks_d[j] = d;
}

// blocks per column for the multi-block counting path: ~128 elements per
// block keeps every block's sweep a few microseconds while n_cols*g
// workgroups fill the 256 CUs
inline int ks_mb_blocks(int b) {
  int g = (b + 127) / 128;
  if (g < 1) g = 1;
  if (g > 128) g = 128;
  return g;
}
constexpr int KS_MB_MAX_G = 128;

// ---------------------------------------------------------------------------
// Host launchers
// ---------------------------------------------------------------------------

namespace {

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

void check_inputs(const torch::Tensor& codes, const torch::Tensor& nums) {
  TORCH_CHECK(codes.is_cuda() && nums.is_cuda(), "inputs must be on GPU");
  TORCH_CHECK(codes.scalar_type() == torch::kInt16, "codes must be int16");
  TORCH_CHECK(nums.scalar_type() == torch::kFloat32, "nums must be float32");
  TORCH_CHECK(codes.is_contiguous() && nums.is_contiguous(), "inputs must be contiguous");
  TORCH_CHECK(codes.size(1) == N_CAT && nums.size(1) == N_NUM, "bad feature counts");
  TORCH_CHECK(codes.size(0) == nums.size(0), "row count mismatch");
}

}  // namespace

std::vector<torch::Tensor> score_forest_pipeline(
    torch::Tensor codes, torch::Tensor nums,
    torch::Tensor cls_nodes, torch::Tensor cls_off,
    torch::Tensor feat_col, torch::Tensor feat_code,
    torch::Tensor medians, int64_t n_onehot,
    torch::Tensor if_nodes, torch::Tensor if_off,
    double if_denom, double if_offset, double if_threshold)
{
  (void)n_onehot;  // encoded in feat_code (>=0 ⇔ one-hot)
  check_inputs(codes, nums);
  const int B = (int)codes.size(0);
  const int t_cls = (int)cls_off.size(0) - 1;
  const int t_if = (int)if_off.size(0) - 1;

  auto opts_f64 = torch::TensorOptions().dtype(torch::kFloat64).device(codes.device());
  auto cls_acc = torch::zeros({B}, opts_f64);
  auto if_acc = torch::zeros({B}, opts_f64);
  auto proba = torch::empty({B}, opts_f64);
  auto iscore = torch::empty({B}, opts_f64);
  auto outlier = torch::empty({B}, opts_f64);

  hipStream_t stream = c10::hip::getCurrentHIPStream();
  const int row_blocks = ceil_div(B, BLOCK);
  // enough blocks to cover the 256 CUs / 8 XCDs even for small batches
  auto tree_chunks = [&](int t) {
    int c = ceil_div(2048, row_blocks);
    return std::max(1, std::min(c, t));
  };

  dim3 g_cls(row_blocks, tree_chunks(t_cls));
  hipLaunchKernelGGL((forest_kernel<false>), g_cls, dim3(BLOCK), 0, stream,
      codes.data_ptr<short>(), nums.data_ptr<float>(), medians.data_ptr<float>(),
      reinterpret_cast<const int4*>(cls_nodes.data_ptr<int>()),
      cls_off.data_ptr<int>(), t_cls,
      feat_col.data_ptr<int>(), feat_code.data_ptr<int>(),
      B, cls_acc.data_ptr<double>());

  dim3 g_if(row_blocks, tree_chunks(t_if));
  hipLaunchKernelGGL((forest_kernel<true>), g_if, dim3(BLOCK), 0, stream,
      codes.data_ptr<short>(), nums.data_ptr<float>(), medians.data_ptr<float>(),
      reinterpret_cast<const int4*>(if_nodes.data_ptr<int>()),
      if_off.data_ptr<int>(), t_if,
      nullptr, nullptr,
      B, if_acc.data_ptr<double>());

  hipLaunchKernelGGL(finalize_kernel, dim3(row_blocks), dim3(BLOCK), 0, stream,
      cls_acc.data_ptr<double>(), if_acc.data_ptr<double>(), B,
      /*cls_kind=*/0, 1.0 / (double)t_cls, 0.0, if_denom, if_offset, if_threshold,
      proba.data_ptr<double>(), iscore.data_ptr<double>(), outlier.data_ptr<double>());
  HIP_CHECK(hipGetLastError());

  return {proba, iscore, outlier};
}

// Prediction-path attributions f64[B, 23] for the classifier forest
// (forest_contrib_kernel). Stateless: not part of ScoreSession or any captured
// graph and shares no staging with the scoring path; runs on the caller's
// current stream, no host sync.
torch::Tensor forest_contrib(
    torch::Tensor codes, torch::Tensor nums,
    torch::Tensor cls_nodes, torch::Tensor cls_node_value,
    torch::Tensor cls_off,
    torch::Tensor feat_col, torch::Tensor feat_code,
    torch::Tensor medians, int64_t cls_kind, int64_t block_target)
{
  check_inputs(codes, nums);
  TORCH_CHECK(block_target >= 1 && block_target <= 65535, "bad block_target");
  auto on_dev = [&](const torch::Tensor& t, torch::ScalarType st, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.device() == codes.device(), name,
                " must be on the inputs' GPU");
    TORCH_CHECK(t.scalar_type() == st && t.is_contiguous(), name,
                " has the wrong dtype or is not contiguous");
  };
  on_dev(nums, torch::kFloat32, "nums");
  on_dev(cls_nodes, torch::kInt32, "cls_nodes");
  on_dev(cls_node_value, torch::kFloat32, "cls_node_value");
  on_dev(cls_off, torch::kInt32, "cls_off");
  on_dev(feat_col, torch::kInt32, "feat_col");
  on_dev(feat_code, torch::kInt32, "feat_code");
  on_dev(medians, torch::kFloat32, "medians");
  TORCH_CHECK(cls_nodes.dim() == 2 && cls_nodes.size(1) == 4, "cls_nodes must be [n, 4]");
  TORCH_CHECK(cls_node_value.dim() == 1 && cls_node_value.size(0) == cls_nodes.size(0),
              "cls_node_value must be index-aligned with cls_nodes");
  TORCH_CHECK(feat_col.numel() == feat_code.numel(), "feat_col/feat_code size mismatch");
  TORCH_CHECK(medians.numel() == N_NUM, "medians must have N_NUM entries");
  TORCH_CHECK(cls_off.numel() >= 2, "forest has no trees");

  c10::hip::HIPGuard guard((c10::DeviceIndex)codes.get_device());
  const int B = (int)codes.size(0);
  const int T = (int)cls_off.size(0) - 1;
  auto contrib = torch::zeros({B, N_SRC},
      torch::TensorOptions().dtype(torch::kFloat64).device(codes.device()));
  if (B == 0) return contrib;

  hipStream_t stream = c10::hip::getCurrentHIPStream();
  const int row_blocks = ceil_div(B, CONTRIB_BLOCK);
  // Fewer tree-chunks than the scorer's grid: every chunk ends in up to 23
  // f64 atomics per thread, so more trees per thread means fewer atomics
  // (block_target is the A/B knob of bench/kernel_micro.py).
  const int chunks = std::max(1, std::min(ceil_div((int)block_target, row_blocks), T));
  const double scale = (cls_kind == 1) ? 1.0 : 1.0 / (double)T;
  hipLaunchKernelGGL(forest_contrib_kernel, dim3(row_blocks, chunks),
      dim3(CONTRIB_BLOCK), 0, stream,
      codes.data_ptr<short>(), nums.data_ptr<float>(), medians.data_ptr<float>(),
      reinterpret_cast<const int4*>(cls_nodes.data_ptr<int>()),
      cls_node_value.data_ptr<float>(), cls_off.data_ptr<int>(), T,
      feat_col.data_ptr<int>(), feat_code.data_ptr<int>(), B, scale,
      contrib.data_ptr<double>());
  HIP_CHECK(hipGetLastError());
  return contrib;
}

// What-if forest sums f64[J, R] for partial dependence (forest_whatif_kernel):
// the raw classifier sum of each of the R sample rows under each of the J
// jobs' overrides. `jobs` is a HOST i32[J, 4] table {player0, bits0, player1,
// bits1}; it is checked here (players in range, distinct, category codes that
// fit the i16 staging) and then copied to the device on the caller's stream.
// Stateless like forest_contrib; the caller has bounds-checked the forest
// tables (engine._check_forest_tables).
torch::Tensor forest_whatif(
    torch::Tensor codes, torch::Tensor nums,
    torch::Tensor cls_nodes, torch::Tensor cls_off,
    torch::Tensor feat_col, torch::Tensor feat_code,
    torch::Tensor medians, torch::Tensor jobs, int64_t block_target)
{
  check_inputs(codes, nums);
  TORCH_CHECK(block_target >= 1 && block_target <= 65535, "bad block_target");
  auto on_dev = [&](const torch::Tensor& t, torch::ScalarType st, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.device() == codes.device(), name,
                " must be on the inputs' GPU");
    TORCH_CHECK(t.scalar_type() == st && t.is_contiguous(), name,
                " has the wrong dtype or is not contiguous");
  };
  on_dev(nums, torch::kFloat32, "nums");
  on_dev(cls_nodes, torch::kInt32, "cls_nodes");
  on_dev(cls_off, torch::kInt32, "cls_off");
  on_dev(feat_col, torch::kInt32, "feat_col");
  on_dev(feat_code, torch::kInt32, "feat_code");
  on_dev(medians, torch::kFloat32, "medians");
  TORCH_CHECK(cls_nodes.dim() == 2 && cls_nodes.size(1) == 4, "cls_nodes must be [n, 4]");
  TORCH_CHECK(feat_col.numel() == feat_code.numel(), "feat_col/feat_code size mismatch");
  TORCH_CHECK(medians.numel() == N_NUM, "medians must have N_NUM entries");
  TORCH_CHECK(cls_off.numel() >= 2, "forest has no trees");
  TORCH_CHECK(!jobs.is_cuda() && jobs.scalar_type() == torch::kInt32 &&
              jobs.is_contiguous() && jobs.dim() == 2 && jobs.size(1) == 4,
              "jobs must be a contiguous host int32 [J, 4] table");

  const int64_t J = jobs.size(0);
  const int64_t R = codes.size(0);
  TORCH_CHECK(J >= 1, "forest_whatif needs at least one job");
  TORCH_CHECK(R >= 1, "forest_whatif needs at least one sample row");
  TORCH_CHECK(J < (int64_t(1) << 31) && R < (int64_t(1) << 31), "too many jobs or rows");
  const int* jb = jobs.data_ptr<int>();
  auto code_ok = [](int player, int bits) {
    return player >= N_CAT || (bits >= -32768 && bits <= 32767);
  };
  for (int64_t j = 0; j < J; ++j) {
    const int p0 = jb[4 * j], p1 = jb[4 * j + 2];
    TORCH_CHECK(p0 >= 0 && p0 < N_SRC, "job ", j, ": player0 out of range");
    TORCH_CHECK(p1 >= -1 && p1 < N_SRC, "job ", j, ": player1 out of range");
    TORCH_CHECK(p0 != p1, "job ", j, ": player0 and player1 must differ");
    TORCH_CHECK(code_ok(p0, jb[4 * j + 1]) && (p1 < 0 || code_ok(p1, jb[4 * j + 3])),
                "job ", j, ": category code does not fit int16");
  }

  c10::hip::HIPGuard guard((c10::DeviceIndex)codes.get_device());
  auto out = torch::empty({J, R},
      torch::TensorOptions().dtype(torch::kFloat64).device(codes.device()));
  auto jobs_dev = jobs.to(codes.device());

  hipStream_t stream = c10::hip::getCurrentHIPStream();
  const int T = (int)cls_off.size(0) - 1;
  const int row_blocks = ceil_div((int)R, WHATIF_BLOCK);
  // One-wave blocks; a block takes more than one job only once the grid
  // passes block_target blocks (restaging 74 B per row is nothing next to a
  // forest walk, and more blocks balance better).
  const int chunks = (int)std::max<int64_t>(
      1, std::min<int64_t>(ceil_div((int)block_target, row_blocks), J));
  hipLaunchKernelGGL(forest_whatif_kernel, dim3(row_blocks, chunks),
      dim3(WHATIF_BLOCK), 0, stream,
      codes.data_ptr<short>(), nums.data_ptr<float>(), medians.data_ptr<float>(),
      reinterpret_cast<const int4*>(cls_nodes.data_ptr<int>()),
      cls_off.data_ptr<int>(), T,
      feat_col.data_ptr<int>(), feat_code.data_ptr<int>(),
      reinterpret_cast<const int4*>(jobs_dev.data_ptr<int>()), (int)J, (int)R,
      out.data_ptr<double>());
  HIP_CHECK(hipGetLastError());
  return out;
}

// Accumulated local effects (forest_ale_kernel): {interval i32[E, R], sums
// f64[E, R, 2]} of the R sample rows under each of the E entries. `players`
// (i32[E], numeric schema indices), `edge_off` (i32[E+1]) and `edges` (f32,
// the entries' edge lists one after the other) are HOST tables; they are
// checked here (players numeric, offsets that span `edges` with 2 to
// ALE_MAX_EDGES edges per entry, edges finite and strictly ascending) and
// then copied to the device on the caller's stream. Stateless like
// forest_whatif; the kernel bounds-checks the forest tables itself.
std::vector<torch::Tensor> forest_ale(
    torch::Tensor codes, torch::Tensor nums,
    torch::Tensor cls_nodes, torch::Tensor cls_off,
    torch::Tensor feat_col, torch::Tensor feat_code,
    torch::Tensor medians, torch::Tensor players,
    torch::Tensor edge_off, torch::Tensor edges, int64_t block_target)
{
  check_inputs(codes, nums);
  TORCH_CHECK(block_target >= 1 && block_target <= 65535, "bad block_target");
  auto on_dev = [&](const torch::Tensor& t, torch::ScalarType st, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.device() == codes.device(), name,
                " must be on the inputs' GPU");
    TORCH_CHECK(t.scalar_type() == st && t.is_contiguous(), name,
                " has the wrong dtype or is not contiguous");
  };
  auto on_host = [&](const torch::Tensor& t, torch::ScalarType st, const char* name) {
    TORCH_CHECK(!t.is_cuda() && t.scalar_type() == st && t.is_contiguous() && t.dim() == 1,
                name, " must be a contiguous one-dimensional host table of its dtype");
  };
  on_dev(nums, torch::kFloat32, "nums");
  on_dev(cls_nodes, torch::kInt32, "cls_nodes");
  on_dev(cls_off, torch::kInt32, "cls_off");
  on_dev(feat_col, torch::kInt32, "feat_col");
  on_dev(feat_code, torch::kInt32, "feat_code");
  on_dev(medians, torch::kFloat32, "medians");
  on_host(players, torch::kInt32, "players");
  on_host(edge_off, torch::kInt32, "edge_off");
  on_host(edges, torch::kFloat32, "edges");
  TORCH_CHECK(cls_nodes.dim() == 2 && cls_nodes.size(1) == 4, "cls_nodes must be [n, 4]");
  TORCH_CHECK(cls_nodes.size(0) < (int64_t(1) << 31), "too many nodes");
  TORCH_CHECK(feat_col.numel() == feat_code.numel(), "feat_col/feat_code size mismatch");
  TORCH_CHECK(medians.numel() == N_NUM, "medians must have N_NUM entries");
  TORCH_CHECK(cls_off.numel() >= 2, "forest has no trees");

  const int64_t E = players.numel();
  const int64_t R = codes.size(0);
  TORCH_CHECK(E >= 1, "forest_ale needs at least one entry");
  TORCH_CHECK(R >= 1, "forest_ale needs at least one sample row");
  TORCH_CHECK(E <= 65535 && R < (int64_t(1) << 31), "too many entries or rows");
  TORCH_CHECK(edge_off.numel() == E + 1, "edge_off must have one entry more than players");
  const int* pl = players.data_ptr<int>();
  const int* eo = edge_off.data_ptr<int>();
  const float* ed = edges.data_ptr<float>();
  TORCH_CHECK(eo[0] == 0 && (int64_t)eo[E] == edges.numel(), "edge_off does not span edges");
  for (int64_t e = 0; e < E; ++e) {
    TORCH_CHECK(pl[e] >= N_CAT && pl[e] < N_SRC, "entry ", e,
                ": player must be a numeric feature (categorical columns have no intervals)");
    const int64_t n = (int64_t)eo[e + 1] - eo[e];
    TORCH_CHECK(n >= 2 && n <= ALE_MAX_EDGES && eo[e] >= 0, "entry ", e,
                ": edge_off must ascend by 2 to ", ALE_MAX_EDGES, " edges per entry");
    for (int64_t i = eo[e]; i < eo[e + 1]; ++i)
      TORCH_CHECK(std::isfinite(ed[i]) && (i == eo[e] || ed[i - 1] < ed[i]), "entry ", e,
                  ": edges must be finite and strictly ascending");
  }

  c10::hip::HIPGuard guard((c10::DeviceIndex)codes.get_device());
  auto dev = codes.device();
  auto interval = torch::empty({E, R}, torch::TensorOptions().dtype(torch::kInt32).device(dev));
  auto sums = torch::empty({E, R, 2}, torch::TensorOptions().dtype(torch::kFloat64).device(dev));
  auto players_dev = players.to(dev);
  auto edge_off_dev = edge_off.to(dev);
  auto edges_dev = edges.to(dev);

  hipStream_t stream = c10::hip::getCurrentHIPStream();
  const int T = (int)cls_off.size(0) - 1;
  const int row_blocks = ceil_div((int)R, ALE_BLOCK);
  // One-wave blocks; a block takes more than one entry only once the grid
  // passes block_target blocks (as forest_whatif).
  const int chunks = (int)std::max<int64_t>(
      1, std::min<int64_t>(ceil_div((int)block_target, row_blocks), E));
  hipLaunchKernelGGL(forest_ale_kernel, dim3(row_blocks, chunks),
      dim3(ALE_BLOCK), 0, stream,
      codes.data_ptr<short>(), nums.data_ptr<float>(), medians.data_ptr<float>(),
      reinterpret_cast<const int4*>(cls_nodes.data_ptr<int>()),
      cls_off.data_ptr<int>(), T, (unsigned)cls_nodes.size(0),
      feat_col.data_ptr<int>(), feat_code.data_ptr<int>(), (unsigned)feat_col.numel(),
      players_dev.data_ptr<int>(), edge_off_dev.data_ptr<int>(), edges_dev.data_ptr<float>(),
      (int)E, (int)R, interval.data_ptr<int>(),
      reinterpret_cast<double2*>(sums.data_ptr<double>()));
  HIP_CHECK(hipGetLastError());
  return {interval, sums};
}

// Permutation importance (forest_permute_kernel): f64[Q, R], the raw
// classifier sum of each of the R sample rows with column perm_player[q]
// taken from donor row perm[q, r]. `perm_player` (i32[Q], schema players,
// equal players adjacent) and `perm` (i32[Q, R]) are HOST tables; they are
// checked here (players in [0, N_SRC), every donor in [0, R)), consecutive
// table rows of one player are grouped into jobs of up to PERM_ILP, and
// both are copied to the device on the caller's stream. Stateless like
// forest_ale; the kernel bounds-checks the forest tables itself.
torch::Tensor forest_permute(
    torch::Tensor codes, torch::Tensor nums,
    torch::Tensor cls_nodes, torch::Tensor cls_off,
    torch::Tensor feat_col, torch::Tensor feat_code,
    torch::Tensor medians, torch::Tensor perm_player,
    torch::Tensor perm, int64_t block_target)
{
  check_inputs(codes, nums);
  TORCH_CHECK(block_target >= 1 && block_target <= 65535, "bad block_target");
  auto on_dev = [&](const torch::Tensor& t, torch::ScalarType st, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.device() == codes.device(), name,
                " must be on the inputs' GPU");
    TORCH_CHECK(t.scalar_type() == st && t.is_contiguous(), name,
                " has the wrong dtype or is not contiguous");
  };
  auto on_host = [&](const torch::Tensor& t, int64_t dim, const char* name) {
    TORCH_CHECK(!t.is_cuda() && t.scalar_type() == torch::kInt32 && t.is_contiguous() &&
                t.dim() == dim, name, " must be a contiguous ", dim,
                "-dimensional host int32 table");
  };
  on_dev(nums, torch::kFloat32, "nums");
  on_dev(cls_nodes, torch::kInt32, "cls_nodes");
  on_dev(cls_off, torch::kInt32, "cls_off");
  on_dev(feat_col, torch::kInt32, "feat_col");
  on_dev(feat_code, torch::kInt32, "feat_code");
  on_dev(medians, torch::kFloat32, "medians");
  on_host(perm_player, 1, "perm_player");
  on_host(perm, 2, "perm");
  TORCH_CHECK(cls_nodes.dim() == 2 && cls_nodes.size(1) == 4, "cls_nodes must be [n, 4]");
  TORCH_CHECK(cls_nodes.size(0) < (int64_t(1) << 31), "too many nodes");
  TORCH_CHECK(feat_col.numel() == feat_code.numel(), "feat_col/feat_code size mismatch");
  TORCH_CHECK(medians.numel() == N_NUM, "medians must have N_NUM entries");
  TORCH_CHECK(cls_off.numel() >= 2, "forest has no trees");

  const int64_t Q = perm_player.numel();
  const int64_t R = codes.size(0);
  TORCH_CHECK(Q >= 1, "forest_permute needs at least one perm_player entry");
  TORCH_CHECK(R >= 1, "forest_permute needs at least one sample row");
  TORCH_CHECK(Q < (int64_t(1) << 31) && R < (int64_t(1) << 31), "too many table or sample rows");
  TORCH_CHECK(perm.size(0) == Q && perm.size(1) == R, "perm must be [", Q, ", ", R,
              "] (one row per perm_player entry, one donor per sample row), got [",
              perm.size(0), ", ", perm.size(1), "]");
  const int* pl = perm_player.data_ptr<int>();
  const int* pm = perm.data_ptr<int>();
  for (int64_t q = 0; q < Q; ++q) {
    TORCH_CHECK(pl[q] >= 0 && pl[q] < N_SRC, "perm_player[", q, "] = ", pl[q],
                " is outside [0, ", N_SRC, ")");
    bool ok = true;
    for (int64_t r = 0; r < R; ++r) ok &= (unsigned)pm[q * R + r] < (unsigned)R;
    TORCH_CHECK(ok, "perm row ", q, " holds a donor outside [0, ", R, ")");
  }

  // jobs {player, q0, n, 0}: runs of one player, cut every PERM_ILP rows
  std::vector<int> jb;
  for (int64_t q = 0; q < Q;) {
    int64_t n = 1;
    while (n < PERM_ILP && q + n < Q && pl[q + n] == pl[q]) ++n;
    jb.insert(jb.end(), {pl[q], (int)q, (int)n, 0});
    q += n;
  }
  const int64_t J = (int64_t)jb.size() / 4;

  c10::hip::HIPGuard guard((c10::DeviceIndex)codes.get_device());
  auto dev = codes.device();
  auto out = torch::empty({Q, R}, torch::TensorOptions().dtype(torch::kFloat64).device(dev));
  auto jobs_dev = torch::from_blob(jb.data(), {J, 4}, torch::kInt32).to(dev);
  auto perm_dev = perm.to(dev);

  hipStream_t stream = c10::hip::getCurrentHIPStream();
  const int T = (int)cls_off.size(0) - 1;
  const int row_blocks = ceil_div((int)R, PERM_BLOCK);
  // One-wave blocks; a block takes more than one job only once the grid
  // passes block_target blocks (as forest_whatif).
  const int chunks = (int)std::max<int64_t>(
      1, std::min<int64_t>(ceil_div((int)block_target, row_blocks), J));
  hipLaunchKernelGGL(forest_permute_kernel, dim3(row_blocks, chunks),
      dim3(PERM_BLOCK), 0, stream,
      codes.data_ptr<short>(), nums.data_ptr<float>(), medians.data_ptr<float>(),
      reinterpret_cast<const int4*>(cls_nodes.data_ptr<int>()),
      cls_off.data_ptr<int>(), T, (unsigned)cls_nodes.size(0),
      feat_col.data_ptr<int>(), feat_code.data_ptr<int>(), (unsigned)feat_col.numel(),
      reinterpret_cast<const int4*>(jobs_dev.data_ptr<int>()), (int)J,
      perm_dev.data_ptr<int>(), (int)Q, (int)R, out.data_ptr<double>());
  HIP_CHECK(hipGetLastError());
  return out;
}

// Anchor rules (forest_anchor_kernel): {counts i32[M], sums}. Row i of the R
// rows to explain has the candidate anchors masks[mask_off[i] ..
// mask_off[i + 1]) (a list may be empty); counts[m] is the number of the S
// sample rows whose composite under mask m has a raw classifier sum > cut,
// and with `want_sums` sums is f64[M, S], those raw sums (an empty tensor
// otherwise). `sat` is i32[R, S] on the device (bit p: sample row b already
// satisfies row i's predicate on player p); `masks` (i32[M], bits 0..N_SRC-1)
// and `mask_off` (i32[R + 1]) are HOST tables: they are checked here, cut
// into jobs of at most `chunk` <= ANCHOR_CHUNK masks of one row and copied to
// the device on the caller's stream. A job's masks share one walk per tree
// and thread, but a job is one block per 64 sample rows, so a launch with few
// masks needs small jobs to fill the device: `chunk` = 0 picks the smallest
// chunk that still leaves `block_target` blocks. Stateless like
// forest_permute; the kernel bounds-checks the forest tables itself.
std::vector<torch::Tensor> forest_anchor(
    torch::Tensor codes, torch::Tensor nums,
    torch::Tensor bg_codes, torch::Tensor bg_nums,
    torch::Tensor cls_nodes, torch::Tensor cls_off,
    torch::Tensor feat_col, torch::Tensor feat_code,
    torch::Tensor medians, torch::Tensor sat,
    torch::Tensor masks, torch::Tensor mask_off,
    double cut, bool want_sums, int64_t chunk, int64_t block_target)
{
  check_inputs(codes, nums);
  check_inputs(bg_codes, bg_nums);
  TORCH_CHECK(chunk >= 0 && chunk <= ANCHOR_CHUNK, "chunk must be in [0, ", ANCHOR_CHUNK, "]");
  TORCH_CHECK(block_target >= 1 && block_target <= 65535, "bad block_target");
  auto on_dev = [&](const torch::Tensor& t, torch::ScalarType st, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.device() == codes.device(), name,
                " must be on the inputs' GPU");
    TORCH_CHECK(t.scalar_type() == st && t.is_contiguous(), name,
                " has the wrong dtype or is not contiguous");
  };
  auto on_host = [&](const torch::Tensor& t, const char* name) {
    TORCH_CHECK(!t.is_cuda() && t.scalar_type() == torch::kInt32 && t.is_contiguous() &&
                t.dim() == 1, name, " must be a contiguous 1-dimensional host int32 table");
  };
  on_dev(nums, torch::kFloat32, "nums");
  on_dev(bg_codes, torch::kInt16, "bg_codes");
  on_dev(bg_nums, torch::kFloat32, "bg_nums");
  on_dev(cls_nodes, torch::kInt32, "cls_nodes");
  on_dev(cls_off, torch::kInt32, "cls_off");
  on_dev(feat_col, torch::kInt32, "feat_col");
  on_dev(feat_code, torch::kInt32, "feat_code");
  on_dev(medians, torch::kFloat32, "medians");
  on_dev(sat, torch::kInt32, "sat");
  on_host(masks, "masks");
  on_host(mask_off, "mask_off");
  TORCH_CHECK(cls_nodes.dim() == 2 && cls_nodes.size(1) == 4, "cls_nodes must be [n, 4]");
  TORCH_CHECK(cls_nodes.size(0) < (int64_t(1) << 31), "too many nodes");
  TORCH_CHECK(feat_col.numel() == feat_code.numel(), "feat_col/feat_code size mismatch");
  TORCH_CHECK(medians.numel() == N_NUM, "medians must have N_NUM entries");
  TORCH_CHECK(cls_off.numel() >= 2, "forest has no trees");
  TORCH_CHECK(std::isfinite(cut), "cut must be finite");

  const int64_t R = codes.size(0);
  const int64_t S = bg_codes.size(0);
  const int64_t M = masks.numel();
  TORCH_CHECK(R >= 1, "forest_anchor needs at least one row");
  TORCH_CHECK(S >= 1, "forest_anchor needs at least one sample row");
  TORCH_CHECK(R < (int64_t(1) << 31) && S < (int64_t(1) << 31) && M < (int64_t(1) << 31),
              "too many rows, sample rows or masks");
  TORCH_CHECK(sat.dim() == 2 && sat.size(0) == R && sat.size(1) == S,
              "sat must be [", R, ", ", S, "] (one word per row and sample row)");
  TORCH_CHECK(mask_off.numel() == R + 1, "mask_off must have one entry per row and one more");
  const int* mo = mask_off.data_ptr<int>();
  const int* mk = masks.data_ptr<int>();
  TORCH_CHECK(mo[0] == 0 && (int64_t)mo[R] == M, "mask_off does not span masks");
  for (int64_t i = 0; i < R; ++i)
    TORCH_CHECK(mo[i + 1] >= mo[i], "mask_off must not decrease");
  for (int64_t m = 0; m < M; ++m)
    TORCH_CHECK((unsigned)mk[m] < (1u << N_SRC), "masks[", m, "] holds a player outside [0, ",
                N_SRC, ")");

  // one block per job and 64-row pass of the sample (up to the grid's limit)
  const int64_t passes = std::min<int64_t>(ceil_div((int)S, ANCHOR_BLOCK), 65535);
  if (chunk == 0)
    chunk = std::max<int64_t>(1, std::min<int64_t>(ANCHOR_CHUNK, M * passes / block_target));
  // jobs {row, first mask, n, 0}: a row's list, cut every `chunk` masks
  const int step = (int)chunk;
  std::vector<int> jb;
  for (int64_t i = 0; i < R; ++i)
    for (int a = mo[i]; a < mo[i + 1]; a += step)
      jb.insert(jb.end(), {(int)i, a, std::min(step, mo[i + 1] - a), 0});
  const int64_t J = (int64_t)jb.size() / 4;

  c10::hip::HIPGuard guard((c10::DeviceIndex)codes.get_device());
  auto dev = codes.device();
  auto counts = torch::empty({passes, M}, torch::TensorOptions().dtype(torch::kInt32).device(dev));
  auto sums = torch::empty({want_sums ? M : 0, S},
                           torch::TensorOptions().dtype(torch::kFloat64).device(dev));
  if (J == 0) return {counts.view({-1}), sums};  // every list is empty
  auto jobs_dev = torch::from_blob(jb.data(), {J, 4}, torch::kInt32).to(dev);
  auto masks_dev = masks.to(dev);

  hipStream_t stream = c10::hip::getCurrentHIPStream();
  const int T = (int)cls_off.size(0) - 1;
  hipLaunchKernelGGL(forest_anchor_kernel, dim3((unsigned)J, (unsigned)passes),
      dim3(ANCHOR_BLOCK), 0, stream,
      codes.data_ptr<short>(), nums.data_ptr<float>(),
      bg_codes.data_ptr<short>(), bg_nums.data_ptr<float>(), medians.data_ptr<float>(),
      reinterpret_cast<const int4*>(cls_nodes.data_ptr<int>()),
      cls_off.data_ptr<int>(), T, (unsigned)cls_nodes.size(0),
      feat_col.data_ptr<int>(), feat_code.data_ptr<int>(), (unsigned)feat_col.numel(),
      reinterpret_cast<const unsigned*>(sat.data_ptr<int>()),
      reinterpret_cast<const unsigned*>(masks_dev.data_ptr<int>()),
      reinterpret_cast<const int4*>(jobs_dev.data_ptr<int>()),
      (int)R, (int)S, (int)M, cut, counts.data_ptr<int>(),
      want_sums ? sums.data_ptr<double>() : nullptr);
  HIP_CHECK(hipGetLastError());
  // a pass's counts are integers: adding the rows is exact in any order
  return {passes == 1 ? counts.view({M}) : counts.sum(0, false, torch::kInt32), sums};
}

// Exact single-feature sweep (forest_sweep_kernel + forest_sweep_search_kernel)
// for counterfactuals. `jobs` is a HOST i32[J, 2] table {row, numeric column},
// `thr_off` a HOST i32[N_NUM+1] table of offsets into `thr` (the sorted
// distinct thresholds of every numeric column, on the device); both are
// checked here and copied to the device on the caller's stream. `node_rank`
// is index-aligned with cls_nodes. `max_depth` is the deepest tree of the
// forest as the caller measured it (the walk's stack bound). Returns
// {rec i32[J,3] = {k0, k_below, k_above}, raw f64[J,3], curves}: curves is
// the ragged f64 buffer (K+1 sums per job, job after job) when `want_curves`
// and an empty tensor otherwise. The caller has bounds-checked the forest
// tables (engine._check_forest_tables).
std::vector<torch::Tensor> forest_sweep(
    torch::Tensor codes, torch::Tensor nums,
    torch::Tensor cls_nodes, torch::Tensor cls_off,
    torch::Tensor feat_col, torch::Tensor feat_code,
    torch::Tensor medians, torch::Tensor node_rank,
    torch::Tensor thr, torch::Tensor thr_off, torch::Tensor jobs,
    double cut, int64_t max_depth, bool want_curves)
{
  check_inputs(codes, nums);
  auto on_dev = [&](const torch::Tensor& t, torch::ScalarType st, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.device() == codes.device(), name,
                " must be on the inputs' GPU");
    TORCH_CHECK(t.scalar_type() == st && t.is_contiguous(), name,
                " has the wrong dtype or is not contiguous");
  };
  on_dev(nums, torch::kFloat32, "nums");
  on_dev(cls_nodes, torch::kInt32, "cls_nodes");
  on_dev(cls_off, torch::kInt32, "cls_off");
  on_dev(feat_col, torch::kInt32, "feat_col");
  on_dev(feat_code, torch::kInt32, "feat_code");
  on_dev(medians, torch::kFloat32, "medians");
  on_dev(node_rank, torch::kInt32, "node_rank");
  on_dev(thr, torch::kFloat32, "thr");
  TORCH_CHECK(cls_nodes.dim() == 2 && cls_nodes.size(1) == 4, "cls_nodes must be [n, 4]");
  TORCH_CHECK(node_rank.dim() == 1 && node_rank.numel() == cls_nodes.size(0),
              "node_rank must hold one rank per classifier node");
  TORCH_CHECK(feat_col.numel() == feat_code.numel(), "feat_col/feat_code size mismatch");
  TORCH_CHECK(medians.numel() == N_NUM, "medians must have N_NUM entries");
  TORCH_CHECK(cls_off.numel() >= 2, "forest has no trees");
  TORCH_CHECK(cls_nodes.size(0) < (int64_t(1) << 31), "too many nodes");
  TORCH_CHECK(max_depth >= 0 && max_depth <= SWEEP_MAX_DEPTH,
              "forest depth ", max_depth, " exceeds the sweep's stack bound ", SWEEP_MAX_DEPTH);
  TORCH_CHECK(std::isfinite(cut), "cut must be finite");
  TORCH_CHECK(!thr_off.is_cuda() && thr_off.scalar_type() == torch::kInt32 &&
              thr_off.is_contiguous() && thr_off.dim() == 1 && thr_off.numel() == N_NUM + 1,
              "thr_off must be a contiguous host int32 [N_NUM+1] table");
  TORCH_CHECK(!jobs.is_cuda() && jobs.scalar_type() == torch::kInt32 &&
              jobs.is_contiguous() && jobs.dim() == 2 && jobs.size(1) == 2,
              "jobs must be a contiguous host int32 [J, 2] table");
  const int* to = thr_off.data_ptr<int>();
  TORCH_CHECK(to[0] == 0 && (int64_t)to[N_NUM] == thr.numel(), "thr_off does not span thr");
  for (int c = 0; c < N_NUM; ++c)
    TORCH_CHECK(to[c + 1] >= to[c], "thr_off must not decrease");

  const int64_t J = jobs.size(0);
  const int64_t R = codes.size(0);
  TORCH_CHECK(J >= 1, "forest_sweep needs at least one job");
  TORCH_CHECK(R >= 1, "forest_sweep needs at least one row");
  TORCH_CHECK(J < (int64_t(1) << 31) && R < (int64_t(1) << 31), "too many jobs or rows");
  const int* jb = jobs.data_ptr<int>();
  auto off_host = torch::empty({J}, torch::TensorOptions().dtype(torch::kInt64));
  int64_t* oh = off_host.data_ptr<int64_t>();
  int64_t total = 0, longest = 0;
  for (int64_t j = 0; j < J; ++j) {
    const int row = jb[2 * j], col = jb[2 * j + 1];
    TORCH_CHECK(row >= 0 && row < R, "job ", j, ": row out of range");
    TORCH_CHECK(col >= 0 && col < N_NUM, "job ", j, ": numeric column out of range");
    const int64_t n_int = (int64_t)(to[col + 1] - to[col]) + 1;
    oh[j] = total;
    total += n_int;
    longest = std::max(longest, n_int);
  }
  const int64_t chunks = (longest + SWEEP_CHUNK - 1) / SWEEP_CHUNK;
  TORCH_CHECK(chunks <= 65535, "a column has too many thresholds for one launch");

  c10::hip::HIPGuard guard((c10::DeviceIndex)codes.get_device());
  auto dev = codes.device();
  auto curves = torch::empty({total}, torch::TensorOptions().dtype(torch::kFloat64).device(dev));
  auto rec = torch::empty({J, 3}, torch::TensorOptions().dtype(torch::kInt32).device(dev));
  auto raw = torch::empty({J, 3}, torch::TensorOptions().dtype(torch::kFloat64).device(dev));
  auto jobs_dev = jobs.to(dev);
  auto off_dev = off_host.to(dev);
  auto thr_off_dev = thr_off.to(dev);
  // thr may be empty (a forest of leaves): never dereferenced then (K = 0)
  hipStream_t stream = c10::hip::getCurrentHIPStream();
  const int T = (int)cls_off.size(0) - 1;
  hipLaunchKernelGGL(forest_sweep_kernel, dim3((unsigned)J, (unsigned)chunks),
      dim3(SWEEP_BLOCK), 0, stream,
      codes.data_ptr<short>(), nums.data_ptr<float>(), medians.data_ptr<float>(),
      reinterpret_cast<const int4*>(cls_nodes.data_ptr<int>()), node_rank.data_ptr<int>(),
      cls_off.data_ptr<int>(), T, (unsigned)cls_nodes.size(0),
      feat_col.data_ptr<int>(), feat_code.data_ptr<int>(), (unsigned)feat_col.numel(),
      thr_off_dev.data_ptr<int>(),
      reinterpret_cast<const int2*>(jobs_dev.data_ptr<int>()),
      reinterpret_cast<const long long*>(off_dev.data_ptr<int64_t>()), (int)J, (int)R,
      curves.data_ptr<double>());
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(forest_sweep_search_kernel, dim3((unsigned)J), dim3(SWEEP_BLOCK), 0, stream,
      nums.data_ptr<float>(), medians.data_ptr<float>(), thr.data_ptr<float>(),
      thr_off_dev.data_ptr<int>(),
      reinterpret_cast<const int2*>(jobs_dev.data_ptr<int>()),
      reinterpret_cast<const long long*>(off_dev.data_ptr<int64_t>()),
      curves.data_ptr<double>(), cut, (int)J, (int)R,
      rec.data_ptr<int>(), raw.data_ptr<double>());
  HIP_CHECK(hipGetLastError());
  if (!want_curves)
    curves = torch::empty({0}, torch::TensorOptions().dtype(torch::kFloat64).device(dev));
  return {rec, raw, curves};
}

// Host-side checks shared by the path-table attributions (forest_shap,
// forest_shap_interactions): inputs and table on one GPU, dtypes, shapes.
static void check_shap_inputs(
    const torch::Tensor& codes, const torch::Tensor& nums,
    const torch::Tensor& leaf_value, const torch::Tensor& leaf_off,
    const torch::Tensor& splits, const torch::Tensor& medians,
    int64_t n_trees, int64_t block_target)
{
  check_inputs(codes, nums);
  TORCH_CHECK(block_target >= 1 && block_target <= 65535, "bad block_target");
  auto on_dev = [&](const torch::Tensor& t, torch::ScalarType st, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.device() == codes.device(), name,
                " must be on the inputs' GPU");
    TORCH_CHECK(t.scalar_type() == st && t.is_contiguous(), name,
                " has the wrong dtype or is not contiguous");
  };
  on_dev(nums, torch::kFloat32, "nums");
  on_dev(leaf_value, torch::kFloat32, "leaf_value");
  on_dev(leaf_off, torch::kInt32, "leaf_off");
  on_dev(splits, torch::kInt32, "splits");
  on_dev(medians, torch::kFloat32, "medians");
  TORCH_CHECK(leaf_value.dim() == 1 && leaf_off.dim() == 1 &&
              leaf_off.size(0) == leaf_value.size(0) + 1,
              "leaf_off must have one entry more than leaf_value");
  TORCH_CHECK(splits.dim() == 2 && splits.size(1) == 4, "splits must be [S, 4]");
  TORCH_CHECK(medians.numel() == N_NUM, "medians must have N_NUM entries");
  TORCH_CHECK(n_trees >= 1, "forest has no trees");
}

// Exact TreeSHAP values f64[B, 23] for the classifier forest
// (forest_shap_kernel) from the path table of pack.build_shap_paths.
// Stateless like forest_contrib; the caller has bounds-checked the table.
torch::Tensor forest_shap(
    torch::Tensor codes, torch::Tensor nums,
    torch::Tensor leaf_value, torch::Tensor leaf_off, torch::Tensor splits,
    torch::Tensor medians, int64_t cls_kind, int64_t n_trees,
    int64_t block_target)
{
  check_shap_inputs(codes, nums, leaf_value, leaf_off, splits, medians, n_trees,
                    block_target);

  c10::hip::HIPGuard guard((c10::DeviceIndex)codes.get_device());
  const int B = (int)codes.size(0);
  const int L = (int)leaf_value.size(0);
  auto shap = torch::zeros({B, N_SRC},
      torch::TensorOptions().dtype(torch::kFloat64).device(codes.device()));
  if (B == 0 || L == 0) return shap;

  hipStream_t stream = c10::hip::getCurrentHIPStream();
  const int row_blocks = ceil_div(B, CONTRIB_BLOCK);
  // As forest_contrib: enough path-chunks to fill the CUs at small B, few
  // enough that the up-to-23 closing atomics per thread stay negligible.
  const int chunks = std::max(1, std::min(ceil_div((int)block_target, row_blocks), L));
  const double scale = (cls_kind == 1) ? 1.0 : 1.0 / (double)n_trees;
  hipLaunchKernelGGL(forest_shap_kernel, dim3(row_blocks, chunks),
      dim3(CONTRIB_BLOCK), 0, stream,
      codes.data_ptr<short>(), nums.data_ptr<float>(), medians.data_ptr<float>(),
      leaf_value.data_ptr<float>(), leaf_off.data_ptr<int>(),
      reinterpret_cast<const int4*>(splits.data_ptr<int>()), L, B, scale,
      shap.data_ptr<double>());
  HIP_CHECK(hipGetLastError());
  return shap;
}

// Exact SHAP interaction values f64[B, 23, 23] for the classifier forest
// (forest_shap_inter_kernel) from the same path table: symmetric, each
// off-diagonal entry half of the pair's interaction index, the diagonal
// left at zero for the caller (engine: phi_i minus the off-diagonal row sum).
// Stateless like forest_shap; the caller has bounds-checked the table.
torch::Tensor forest_shap_interactions(
    torch::Tensor codes, torch::Tensor nums,
    torch::Tensor leaf_value, torch::Tensor leaf_off, torch::Tensor splits,
    torch::Tensor medians, int64_t cls_kind, int64_t n_trees,
    int64_t block_target)
{
  check_shap_inputs(codes, nums, leaf_value, leaf_off, splits, medians, n_trees,
                    block_target);

  c10::hip::HIPGuard guard((c10::DeviceIndex)codes.get_device());
  const int B = (int)codes.size(0);
  const int L = (int)leaf_value.size(0);
  auto upper = torch::zeros({B, N_SRC, N_SRC},
      torch::TensorOptions().dtype(torch::kFloat64).device(codes.device()));
  if (B == 0 || L == 0) return upper;

  hipStream_t stream = c10::hip::getCurrentHIPStream();
  const int row_blocks = ceil_div(B, SHAPI_ROWS);
  // forest_shap's grid rule: path-chunks fill the CUs at small B; every
  // chunk ends in up to 253 atomics per row
  const int chunks = std::max(1, std::min(ceil_div((int)block_target, row_blocks), L));
  const double scale = (cls_kind == 1) ? 1.0 : 1.0 / (double)n_trees;
  hipLaunchKernelGGL(forest_shap_inter_kernel, dim3(row_blocks, chunks),
      dim3(SHAPI_BLOCK), 0, stream,
      codes.data_ptr<short>(), nums.data_ptr<float>(), medians.data_ptr<float>(),
      leaf_value.data_ptr<float>(), leaf_off.data_ptr<int>(),
      reinterpret_cast<const int4*>(splits.data_ptr<int>()), L, B, 0.5 * scale,
      upper.data_ptr<double>());
  HIP_CHECK(hipGetLastError());
  // the kernel fills the strict upper triangle; x + x^T is bit-symmetric
  return upper + upper.transpose(1, 2);
}

// Interventional Shapley values f64[B, 23] of the classifier forest against
// the background rows (forest_ishap_kernel), from the same path table.
// Stateless like forest_shap; the caller has bounds-checked the table
// (engine._check_shap_paths: record players, at most N_SRC groups per path).
torch::Tensor forest_ishap(
    torch::Tensor codes, torch::Tensor nums,
    torch::Tensor bg_codes, torch::Tensor bg_nums,
    torch::Tensor leaf_value, torch::Tensor leaf_off, torch::Tensor splits,
    torch::Tensor medians, int64_t cls_kind, int64_t n_trees,
    int64_t block_target)
{
  check_inputs(codes, nums);
  TORCH_CHECK(block_target >= 1 && block_target <= 65535, "bad block_target");
  auto on_dev = [&](const torch::Tensor& t, torch::ScalarType st, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.device() == codes.device(), name,
                " must be on the inputs' GPU");
    TORCH_CHECK(t.scalar_type() == st && t.is_contiguous(), name,
                " has the wrong dtype or is not contiguous");
  };
  on_dev(nums, torch::kFloat32, "nums");
  on_dev(bg_codes, torch::kInt16, "bg_codes");
  on_dev(bg_nums, torch::kFloat32, "bg_nums");
  on_dev(leaf_value, torch::kFloat32, "leaf_value");
  on_dev(leaf_off, torch::kInt32, "leaf_off");
  on_dev(splits, torch::kInt32, "splits");
  on_dev(medians, torch::kFloat32, "medians");
  TORCH_CHECK(bg_codes.dim() == 2 && bg_codes.size(1) == N_CAT,
              "bg_codes must be [R, N_CAT]");
  TORCH_CHECK(bg_nums.dim() == 2 && bg_nums.size(1) == N_NUM &&
              bg_nums.size(0) == bg_codes.size(0),
              "bg_nums must be [R, N_NUM] with bg_codes' R");
  TORCH_CHECK(bg_codes.size(0) >= 1 && bg_codes.size(0) <= ISHAP_MAX_BACKGROUND,
              "the background sample must have 1..", ISHAP_MAX_BACKGROUND, " rows");
  TORCH_CHECK(leaf_value.dim() == 1 && leaf_off.dim() == 1 &&
              leaf_off.size(0) == leaf_value.size(0) + 1,
              "leaf_off must have one entry more than leaf_value");
  TORCH_CHECK(splits.dim() == 2 && splits.size(1) == 4, "splits must be [S, 4]");
  TORCH_CHECK(medians.numel() == N_NUM, "medians must have N_NUM entries");
  TORCH_CHECK(n_trees >= 1, "forest has no trees");

  c10::hip::HIPGuard guard((c10::DeviceIndex)codes.get_device());
  const int B = (int)codes.size(0);
  const int R = (int)bg_codes.size(0);
  const int L = (int)leaf_value.size(0);
  auto phi = torch::zeros({B, N_SRC},
      torch::TensorOptions().dtype(torch::kFloat64).device(codes.device()));
  if (B == 0 || L == 0) return phi;

  hipStream_t stream = c10::hip::getCurrentHIPStream();
  const int row_blocks = ceil_div(B, CONTRIB_BLOCK);
  // forest_shap's grid rule: path-chunks fill the CUs at small B
  const int chunks = std::max(1, std::min(ceil_div((int)block_target, row_blocks), L));
  const double scale = (cls_kind == 1) ? 1.0 : 1.0 / (double)n_trees;
  hipLaunchKernelGGL(forest_ishap_kernel, dim3(row_blocks, chunks),
      dim3(CONTRIB_BLOCK), 0, stream,
      codes.data_ptr<short>(), nums.data_ptr<float>(),
      bg_codes.data_ptr<short>(), bg_nums.data_ptr<float>(),
      medians.data_ptr<float>(),
      leaf_value.data_ptr<float>(), leaf_off.data_ptr<int>(),
      reinterpret_cast<const int4*>(splits.data_ptr<int>()), L, B, R,
      scale / (double)R, phi.data_ptr<double>());
  HIP_CHECK(hipGetLastError());
  return phi;
}

// ---------------------------------------------------------------------------
// Histogram gradient-boosted-tree trainer (creditcore/models/hgbt.py).
//
// One tree level = three launches: hgbt_hist_kernel (per-(node, bin) integer
// sums of the fixed-point gradients), hgbt_split_kernel (best split per node)
// and hgbt_route_kernel (rows move to their child). Gradients arrive as int32
// fixed point with HGBT_SHIFT fractional bits, so every histogram sum is an
// integer and the result does not depend on the order atomics land in; the
// CPU reference (ops/cpu_ref.py hgbt_*_cpu) must match bit for bit.
//
// Layouts: bins u8[F, N] column-major (feature-major), ragged bin offsets
// bin_off i32[F+1]; per-row node id i32[N] = slot of the row's node among
// the level's open nodes, negative once the row sits in a leaf; histogram
// i64[n_nodes, 3, total_bins] with planes {sum g, sum h, row count}.
// ---------------------------------------------------------------------------

#define HGBT_BLOCK 256
#define HGBT_SHIFT 20
#define HGBT_MAX_BINS 256
#define HGBT_REC 9  // split record, i64 words: gain bits, feat, bin, GL, HL, CL, G, H, C
// int32 LDS partials: |gq| <= 2^HGBT_SHIFT per row, so a block may sum at most
// this many rows before a partial could leave int32.
static constexpr int64_t HGBT_MAX_ROWS_PER_BLOCK = (int64_t(1) << (31 - HGBT_SHIFT)) - 1;
static constexpr size_t HGBT_LDS_BYTES_MAX = 160 * 1024 - 1024;  // gfx950 LDS/CU

// grid = (row blocks, feature groups). lds_entries > 0: the block's
// (n_nodes x 3 x group bins) slab is summed in LDS with int32 atomics and
// flushed with one global atomic per non-zero entry; lds_entries == 0 (deep
// levels, slab larger than LDS): int64 atomics straight to global memory.
// Every offset read from bin_off / grp_off is range-checked before use, so
// bad table contents skip work instead of writing out of bounds.
__global__ __launch_bounds__(HGBT_BLOCK) void hgbt_hist_kernel(
    const uint8_t* __restrict__ bins, const int* __restrict__ bin_off,
    const int* __restrict__ grp_off, const int* __restrict__ node,
    const int* __restrict__ gq, const int* __restrict__ hq,
    long long n_rows, int n_feat, int n_nodes, int total_bins,
    int rows_per_block, int lds_entries,
    unsigned long long* __restrict__ hist)
{
  extern __shared__ int hgbt_lds[];
  const int tid = threadIdx.x;
  const int f0 = grp_off[blockIdx.y], f1 = grp_off[blockIdx.y + 1];
  if (f0 < 0 || f1 > n_feat || f0 >= f1) return;
  const int b0 = bin_off[f0];
  const int gb = bin_off[f1] - b0;  // bins of this feature group
  if (b0 < 0 || gb <= 0 || (long long)b0 + gb > total_bins) return;
  const bool use_lds = lds_entries > 0;
  const long long slab = (long long)n_nodes * 3 * gb;
  if (use_lds) {
    if (slab > lds_entries) return;  // host sizes the allocation from the same tables
    for (int i = tid; i < (int)slab; i += HGBT_BLOCK) hgbt_lds[i] = 0;
    __syncthreads();
  }

  const long long r0 = (long long)blockIdx.x * rows_per_block;
  const long long r1 = min(r0 + (long long)rows_per_block, n_rows);
  // consecutive lanes take consecutive rows: the u8 column reads coalesce
  for (long long r = r0 + tid; r < r1; r += HGBT_BLOCK) {
    const int nd = node[r];
    if (nd < 0 || nd >= n_nodes) continue;  // row already in a leaf
    const int g = gq[r], h = hq[r];
    for (int f = f0; f < f1; ++f) {
      const int fb = bin_off[f];
      const int nb = bin_off[f + 1] - fb;
      if (fb < b0 || nb <= 0 || fb + nb > b0 + gb) continue;
      const int b = bins[(size_t)f * (size_t)n_rows + (size_t)r];
      if (b >= nb) continue;
      if (use_lds) {
        int* p = hgbt_lds + (size_t)nd * 3 * gb + (fb - b0) + b;
        atomicAdd(p, g);
        atomicAdd(p + gb, h);
        atomicAdd(p + 2 * gb, 1);
      } else {
        unsigned long long* p = hist + (size_t)nd * 3 * total_bins + fb + b;
        atomicAdd(p, (unsigned long long)(long long)g);
        atomicAdd(p + total_bins, (unsigned long long)(long long)h);
        atomicAdd(p + 2 * (size_t)total_bins, 1ull);
      }
    }
  }

  if (use_lds) {
    __syncthreads();
    for (int i = tid; i < (int)slab; i += HGBT_BLOCK) {
      const int v = hgbt_lds[i];
      if (v == 0) continue;
      const int plane = i / gb;  // node * 3 + {g, h, count}
      const int b = i - plane * gb;
      atomicAdd(hist + (size_t)plane * total_bins + b0 + b,
                (unsigned long long)(long long)v);
    }
  }
}

// Split gain from the integer sums, in f64. The operation order is the one
// hgbt_split_cpu uses, and contraction is off: an FMA here would round
// differently from numpy and break the bit-exact agreement.
__device__ __forceinline__ double hgbt_gain(
    long long GL, long long HL, long long G, long long H, double lam)
{
#pragma clang fp contract(off)
  const double sc = 1.0 / (double)(1 << HGBT_SHIFT);
  const double gl = (double)GL * sc, hl = (double)HL * sc;
  const double gr = (double)(G - GL) * sc, hr = (double)(H - HL) * sc;
  const double g = (double)G * sc, h = (double)H * sc;
  const double a = (gl * gl) / (hl + lam);
  const double b = (gr * gr) / (hr + lam);
  const double c = (g * g) / (h + lam);
  return (a + b) - c;
}

struct HgbtBest {
  double gain;
  int feat, bin;
  long long GL, HL, CL;
};

// highest gain, then lowest feature, then lowest bin; feat < 0 = no split yet
__device__ __forceinline__ bool hgbt_better(const HgbtBest& a, const HgbtBest& b) {
  if (a.feat < 0) return false;
  if (b.feat < 0) return true;
  if (a.gain != b.gain) return a.gain > b.gain;
  if (a.feat != b.feat) return a.feat < b.feat;
  return a.bin < b.bin;
}

__device__ __forceinline__ HgbtBest hgbt_shfl_xor(const HgbtBest& v, int m) {
  HgbtBest o;
  o.gain = __shfl_xor(v.gain, m);
  o.feat = __shfl_xor(v.feat, m);
  o.bin = __shfl_xor(v.bin, m);
  o.GL = __shfl_xor(v.GL, m);
  o.HL = __shfl_xor(v.HL, m);
  o.CL = __shfl_xor(v.CL, m);
  return o;
}

// One block per open node; each of its 4 wavefronts takes every 4th feature.
// A lane owns 4 consecutive bins (64 x 4 = HGBT_MAX_BINS), scans them, and a
// wave-wide shuffle scan of the lane totals gives the prefix sums. "bin <= b
// goes left" is valid when both sides keep min_leaf rows and the gain is > 0.
__global__ __launch_bounds__(HGBT_BLOCK) void hgbt_split_kernel(
    const long long* __restrict__ hist, const int* __restrict__ bin_off,
    int n_feat, int total_bins, double lam, long long min_leaf,
    long long* __restrict__ out)
{
  __shared__ HgbtBest wave_best[HGBT_BLOCK / 64];
  __shared__ long long wave_tot[HGBT_BLOCK / 64][3];
  const int k = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long* hg = hist + (size_t)k * 3 * total_bins;
  const long long* hh = hg + total_bins;
  const long long* hc = hh + total_bins;

  HgbtBest best;
  best.gain = 0.0; best.feat = -1; best.bin = 0; best.GL = best.HL = best.CL = 0;
  long long G = 0, H = 0, C = 0;
  for (int f = wave; f < n_feat; f += HGBT_BLOCK / 64) {
    const int fb = bin_off[f];
    const int nb = bin_off[f + 1] - fb;
    if (fb < 0 || nb <= 0 || nb > HGBT_MAX_BINS || fb + nb > total_bins) continue;
    long long pg[4], ph[4], pc[4];
    long long sg = 0, sh = 0, sc = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int b = lane * 4 + j;
      if (b < nb) { sg += hg[fb + b]; sh += hh[fb + b]; sc += hc[fb + b]; }
      pg[j] = sg; ph[j] = sh; pc[j] = sc;
    }
    // inclusive scan of the lane totals across the wavefront
    long long ig = sg, ih = sh, ic = sc;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long tg = __shfl_up(ig, d), th = __shfl_up(ih, d), tc = __shfl_up(ic, d);
      if (lane >= d) { ig += tg; ih += th; ic += tc; }
    }
    // every feature sees every open row once: the totals are the node's own
    G = __shfl(ig, 63); H = __shfl(ih, 63); C = __shfl(ic, 63);
    const long long og = ig - sg, oh = ih - sh, oc = ic - sc;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int b = lane * 4 + j;
      if (b >= nb) continue;
      const long long CL = oc + pc[j];
      if (CL < min_leaf || C - CL < min_leaf) continue;
      HgbtBest c;
      c.GL = og + pg[j]; c.HL = oh + ph[j]; c.CL = CL;
      c.feat = f; c.bin = b;
      c.gain = hgbt_gain(c.GL, c.HL, G, H, lam);
      if (!(c.gain > 0.0)) continue;
      if (hgbt_better(c, best)) best = c;
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const HgbtBest o = hgbt_shfl_xor(best, m);
    if (hgbt_better(o, best)) best = o;
  }
  if (lane == 0) {
    wave_best[wave] = best;
    wave_tot[wave][0] = G; wave_tot[wave][1] = H; wave_tot[wave][2] = C;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < HGBT_BLOCK / 64; ++w)
      if (hgbt_better(wave_best[w], best)) best = wave_best[w];
    // wave 0 always scans feature 0 (n_feat >= 1), so its totals are set
    long long* o = out + (size_t)k * HGBT_REC;
    o[0] = __double_as_longlong(best.feat < 0 ? 0.0 : best.gain);
    o[1] = best.feat; o[2] = best.bin;
    o[3] = best.GL; o[4] = best.HL; o[5] = best.CL;
    o[6] = wave_tot[0][0]; o[7] = wave_tot[0][1]; o[8] = wave_tot[0][2];
  }
}

// Monotone-constrained split search (models/hgbt.py, "monotone constraints").
// A side with sums (g, d = h + lam) and the node's weight bounds [lo, hi]
// takes the clamped Newton weight w and scores -(2 g w + d w^2), which is
// g^2/d when the clamp is idle. Operation order is hgbt_split_mono_cpu's and
// contraction is off (see hgbt_gain). The clamp is written as compares so
// that it selects the same operand as the reference's np.where.
__device__ __forceinline__ double hgbt_mono_score(
    double g, double d, double lo, double hi, double* w_out)
{
#pragma clang fp contract(off)
  double w = -g / d;
  w = w < lo ? lo : w;
  w = w > hi ? hi : w;
  *w_out = w;
  const double a = (2.0 * g) * w;
  const double b = (d * w) * w;
  return -(a + b);
}

// hgbt_split_kernel's decomposition (one block per open node, 4 wavefronts
// striding the features, 4 bins per lane, shuffle scan, xor-shuffle + LDS
// reduction) with the bounds-propagation rule of XGBoost-hist / LightGBM
// "basic": mono[f] in {-1, 0, +1} is feature f's sign, bounds[k] = {lo, hi}
// the leaf-weight interval of open node k. Left, right and parent are clamped
// to the node's interval; a candidate also needs d_L > 0, d_R > 0 and, on a
// signed feature, w_L <= w_R (+1) or w_L >= w_R (-1).
__global__ __launch_bounds__(HGBT_BLOCK) void hgbt_split_mono_kernel(
    const long long* __restrict__ hist, const int* __restrict__ bin_off,
    const int* __restrict__ mono, const double* __restrict__ bounds,
    int n_feat, int total_bins, double lam, long long min_leaf,
    long long* __restrict__ out)
{
#pragma clang fp contract(off)
  __shared__ HgbtBest wave_best[HGBT_BLOCK / 64];
  __shared__ long long wave_tot[HGBT_BLOCK / 64][3];
  const int k = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long* hg = hist + (size_t)k * 3 * total_bins;
  const long long* hh = hg + total_bins;
  const long long* hc = hh + total_bins;
  const double lo = bounds[2 * (size_t)k], hi = bounds[2 * (size_t)k + 1];
  const double scale = 1.0 / (double)(1 << HGBT_SHIFT);

  HgbtBest best;
  best.gain = 0.0; best.feat = -1; best.bin = 0; best.GL = best.HL = best.CL = 0;
  long long G = 0, H = 0, C = 0;
  for (int f = wave; f < n_feat; f += HGBT_BLOCK / 64) {
    const int fb = bin_off[f];
    const int nb = bin_off[f + 1] - fb;
    if (fb < 0 || nb <= 0 || nb > HGBT_MAX_BINS || fb + nb > total_bins) continue;
    const int sign = mono[f];
    long long pg[4], ph[4], pc[4];
    long long sg = 0, sh = 0, sc = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int b = lane * 4 + j;
      if (b < nb) { sg += hg[fb + b]; sh += hh[fb + b]; sc += hc[fb + b]; }
      pg[j] = sg; ph[j] = sh; pc[j] = sc;
    }
    // inclusive scan of the lane totals across the wavefront
    long long ig = sg, ih = sh, ic = sc;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long tg = __shfl_up(ig, d), th = __shfl_up(ih, d), tc = __shfl_up(ic, d);
      if (lane >= d) { ig += tg; ih += th; ic += tc; }
    }
    G = __shfl(ig, 63); H = __shfl(ih, 63); C = __shfl(ic, 63);
    // parent weight and score: once per feature, from the node totals
    double w_p;
    const double s_p =
        hgbt_mono_score((double)G * scale, (double)H * scale + lam, lo, hi, &w_p);
    const long long og = ig - sg, oh = ih - sh, oc = ic - sc;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int b = lane * 4 + j;
      if (b >= nb) continue;
      const long long CL = oc + pc[j];
      if (CL < min_leaf || C - CL < min_leaf) continue;
      HgbtBest c;
      c.GL = og + pg[j]; c.HL = oh + ph[j]; c.CL = CL;
      c.feat = f; c.bin = b;
      const double d_l = (double)c.HL * scale + lam;
      const double d_r = (double)(H - c.HL) * scale + lam;
      if (!(d_l > 0.0) || !(d_r > 0.0)) continue;
      double w_l, w_r;
      const double s_l = hgbt_mono_score((double)c.GL * scale, d_l, lo, hi, &w_l);
      const double s_r = hgbt_mono_score((double)(G - c.GL) * scale, d_r, lo, hi, &w_r);
      c.gain = (s_l + s_r) - s_p;
      if (!(c.gain > 0.0)) continue;
      if (sign > 0 && !(w_l <= w_r)) continue;
      if (sign < 0 && !(w_l >= w_r)) continue;
      if (hgbt_better(c, best)) best = c;
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const HgbtBest o = hgbt_shfl_xor(best, m);
    if (hgbt_better(o, best)) best = o;
  }
  if (lane == 0) {
    wave_best[wave] = best;
    wave_tot[wave][0] = G; wave_tot[wave][1] = H; wave_tot[wave][2] = C;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < HGBT_BLOCK / 64; ++w)
      if (hgbt_better(wave_best[w], best)) best = wave_best[w];
    // wave 0 always scans feature 0 (n_feat >= 1), so its totals are set
    long long* o = out + (size_t)k * HGBT_REC;
    o[0] = __double_as_longlong(best.feat < 0 ? 0.0 : best.gain);
    o[1] = best.feat; o[2] = best.bin;
    o[3] = best.GL; o[4] = best.HL; o[5] = best.CL;
    o[6] = wave_tot[0][0]; o[7] = wave_tot[0][1]; o[8] = wave_tot[0][2];
  }
}

// table[k] = {feat, bin, left, right} for open node k: rows with
// bins[feat] <= bin take `left`, the others `right`; feat < 0 closes the node
// and every row takes `left`. A target >= 0 is the child's slot in the next
// level, a negative one encodes leaf node t of the tree as -(t + 1).
__global__ __launch_bounds__(HGBT_BLOCK) void hgbt_route_kernel(
    const uint8_t* __restrict__ bins, const int4* __restrict__ table,
    long long n_rows, int n_feat, int n_nodes, int* __restrict__ node)
{
  const long long r = (long long)blockIdx.x * HGBT_BLOCK + threadIdx.x;
  if (r >= n_rows) return;
  const int nd = node[r];
  if (nd < 0 || nd >= n_nodes) return;
  const int4 t = table[nd];
  if (t.x < 0) {
    node[r] = t.z;
  } else if (t.x < n_feat) {
    const int b = bins[(size_t)t.x * (size_t)n_rows + (size_t)r];
    node[r] = (b <= t.y) ? t.z : t.w;
  }
}

void hgbt_check(const torch::Tensor& t, const torch::Tensor& like,
                torch::ScalarType st, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device(), name,
              " must be on the bin matrix's GPU");
  TORCH_CHECK(t.scalar_type() == st && t.is_contiguous(), name,
              " has the wrong dtype or is not contiguous");
}

// Level histogram i64[n_nodes, 3, total_bins]. lds_entries is the int32
// entry count of the largest feature group's slab (n_nodes * 3 * group bins),
// or 0 to take the direct-global path.
torch::Tensor hgbt_hist(
    torch::Tensor bins, torch::Tensor bin_off, torch::Tensor grp_off,
    torch::Tensor node, torch::Tensor gq, torch::Tensor hq,
    int64_t n_nodes, int64_t total_bins, int64_t lds_entries,
    int64_t rows_per_block)
{
  TORCH_CHECK(bins.is_cuda() && bins.scalar_type() == torch::kUInt8 &&
              bins.dim() == 2 && bins.is_contiguous(),
              "bins must be a contiguous u8[F, N] GPU tensor");
  const int64_t F = bins.size(0), N = bins.size(1);
  hgbt_check(bin_off, bins, torch::kInt32, "bin_off");
  hgbt_check(grp_off, bins, torch::kInt32, "grp_off");
  hgbt_check(node, bins, torch::kInt32, "node");
  hgbt_check(gq, bins, torch::kInt32, "gq");
  hgbt_check(hq, bins, torch::kInt32, "hq");
  TORCH_CHECK(F >= 1 && F <= 65535, "feature count out of range");
  TORCH_CHECK(bin_off.dim() == 1 && bin_off.size(0) == F + 1, "bin_off must be i32[F+1]");
  TORCH_CHECK(grp_off.dim() == 1 && grp_off.size(0) >= 2 && grp_off.size(0) <= F + 1,
              "grp_off must be i32[groups+1]");
  TORCH_CHECK(node.numel() == N && gq.numel() == N && hq.numel() == N,
              "node, gq and hq must have one entry per row");
  TORCH_CHECK(n_nodes >= 1 && total_bins >= 1 &&
              total_bins <= F * HGBT_MAX_BINS &&
              n_nodes * 3 * total_bins < (int64_t(1) << 31),
              "histogram shape out of range");
  TORCH_CHECK(rows_per_block >= 1 && rows_per_block <= HGBT_MAX_ROWS_PER_BLOCK,
              "rows_per_block must keep int32 LDS partials in range (<= ",
              HGBT_MAX_ROWS_PER_BLOCK, ")");
  TORCH_CHECK(lds_entries >= 0 &&
              (size_t)lds_entries * sizeof(int) <= HGBT_LDS_BYTES_MAX,
              "LDS slab larger than the CU's LDS");

  c10::hip::HIPGuard guard((c10::DeviceIndex)bins.get_device());
  auto hist = torch::zeros({n_nodes, 3, total_bins},
      torch::TensorOptions().dtype(torch::kInt64).device(bins.device()));
  if (N == 0) return hist;
  const int64_t row_blocks = (N + rows_per_block - 1) / rows_per_block;
  TORCH_CHECK(row_blocks < (int64_t(1) << 31), "too many rows");

  static bool lds_opt_in = false;
  if (!lds_opt_in) {  // dynamic LDS above 64 KiB needs the opt-in once
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&hgbt_hist_kernel),
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)HGBT_LDS_BYTES_MAX));
    lds_opt_in = true;
  }
  hipStream_t stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(hgbt_hist_kernel,
      dim3((unsigned)row_blocks, (unsigned)(grp_off.size(0) - 1)), dim3(HGBT_BLOCK),
      (size_t)lds_entries * sizeof(int), stream,
      bins.data_ptr<uint8_t>(), bin_off.data_ptr<int>(), grp_off.data_ptr<int>(),
      node.data_ptr<int>(), gq.data_ptr<int>(), hq.data_ptr<int>(),
      (long long)N, (int)F, (int)n_nodes, (int)total_bins, (int)rows_per_block,
      (int)lds_entries,
      reinterpret_cast<unsigned long long*>(hist.data_ptr<int64_t>()));
  HIP_CHECK(hipGetLastError());
  return hist;
}

// Best split per open node: i64[n_nodes, HGBT_REC] records.
torch::Tensor hgbt_split(torch::Tensor hist, torch::Tensor bin_off,
                         double lam, int64_t min_leaf)
{
  TORCH_CHECK(hist.is_cuda() && hist.scalar_type() == torch::kInt64 &&
              hist.dim() == 3 && hist.size(1) == 3 && hist.is_contiguous(),
              "hist must be a contiguous i64[n_nodes, 3, total_bins] GPU tensor");
  hgbt_check(bin_off, hist, torch::kInt32, "bin_off");
  TORCH_CHECK(bin_off.dim() == 1 && bin_off.size(0) >= 2, "bin_off must be i32[F+1]");
  TORCH_CHECK(min_leaf >= 1, "min_leaf must be >= 1");
  c10::hip::HIPGuard guard((c10::DeviceIndex)hist.get_device());
  const int64_t K = hist.size(0);
  auto out = torch::zeros({K, HGBT_REC},
      torch::TensorOptions().dtype(torch::kInt64).device(hist.device()));
  if (K == 0) return out;
  hipStream_t stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(hgbt_split_kernel, dim3((unsigned)K), dim3(HGBT_BLOCK), 0, stream,
      reinterpret_cast<const long long*>(hist.data_ptr<int64_t>()),
      bin_off.data_ptr<int>(), (int)(bin_off.size(0) - 1), (int)hist.size(2), lam, (long long)min_leaf,
      reinterpret_cast<long long*>(out.data_ptr<int64_t>()));
  HIP_CHECK(hipGetLastError());
  return out;
}

// Best split per open node under monotone constraints: mono i32[F] holds the
// sign of every feature (only the sign is read), bounds f64[n_nodes, 2] the
// {lo, hi} leaf-weight interval of every open node. Records as hgbt_split.
torch::Tensor hgbt_split_mono(torch::Tensor hist, torch::Tensor bin_off,
                              double lam, int64_t min_leaf,
                              torch::Tensor mono, torch::Tensor bounds)
{
  TORCH_CHECK(hist.is_cuda() && hist.scalar_type() == torch::kInt64 &&
              hist.dim() == 3 && hist.size(1) == 3 && hist.is_contiguous(),
              "hist must be a contiguous i64[n_nodes, 3, total_bins] GPU tensor");
  hgbt_check(bin_off, hist, torch::kInt32, "bin_off");
  TORCH_CHECK(bin_off.dim() == 1 && bin_off.size(0) >= 2, "bin_off must be i32[F+1]");
  TORCH_CHECK(min_leaf >= 1, "min_leaf must be >= 1");
  const int64_t K = hist.size(0), F = bin_off.size(0) - 1;
  hgbt_check(mono, hist, torch::kInt32, "mono");
  TORCH_CHECK(mono.dim() == 1 && mono.size(0) == F, "mono must be i32[F]");
  hgbt_check(bounds, hist, torch::kFloat64, "bounds");
  TORCH_CHECK(bounds.dim() == 2 && bounds.size(0) == K && bounds.size(1) == 2,
              "bounds must be f64[n_nodes, 2]");
  c10::hip::HIPGuard guard((c10::DeviceIndex)hist.get_device());
  auto out = torch::zeros({K, HGBT_REC},
      torch::TensorOptions().dtype(torch::kInt64).device(hist.device()));
  if (K == 0) return out;
  {  // K pairs: one small copy, checked on the host
    const auto host = bounds.cpu();
    const double* b = host.data_ptr<double>();
    for (int64_t k = 0; k < K; ++k)
      TORCH_CHECK(b[2 * k] <= b[2 * k + 1],
                  "bounds need lo <= hi and no NaN (node ", k, ")");
  }
  hipStream_t stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(hgbt_split_mono_kernel, dim3((unsigned)K), dim3(HGBT_BLOCK), 0, stream,
      reinterpret_cast<const long long*>(hist.data_ptr<int64_t>()),
      bin_off.data_ptr<int>(), mono.data_ptr<int>(), bounds.data_ptr<double>(),
      (int)F, (int)hist.size(2), lam, (long long)min_leaf,
      reinterpret_cast<long long*>(out.data_ptr<int64_t>()));
  HIP_CHECK(hipGetLastError());
  return out;
}

// Move every open row to its child (in place on `node`).
void hgbt_route(torch::Tensor bins, torch::Tensor table, torch::Tensor node)
{
  TORCH_CHECK(bins.is_cuda() && bins.scalar_type() == torch::kUInt8 &&
              bins.dim() == 2 && bins.is_contiguous(),
              "bins must be a contiguous u8[F, N] GPU tensor");
  hgbt_check(table, bins, torch::kInt32, "table");
  hgbt_check(node, bins, torch::kInt32, "node");
  TORCH_CHECK(table.dim() == 2 && table.size(1) == 4, "table must be i32[n_nodes, 4]");
  const int64_t N = bins.size(1);
  TORCH_CHECK(node.numel() == N, "node must have one entry per row");
  if (N == 0 || table.size(0) == 0) return;
  const int64_t blocks = (N + HGBT_BLOCK - 1) / HGBT_BLOCK;
  TORCH_CHECK(blocks < (int64_t(1) << 31), "too many rows");
  c10::hip::HIPGuard guard((c10::DeviceIndex)bins.get_device());
  hipStream_t stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(hgbt_route_kernel, dim3((unsigned)blocks), dim3(HGBT_BLOCK), 0, stream,
      bins.data_ptr<uint8_t>(), reinterpret_cast<const int4*>(table.data_ptr<int>()),
      (long long)N, (int)bins.size(0), (int)table.size(0), node.data_ptr<int>());
  HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// Feature binning on the device (hgbt.bin_features_gpu): what both trainers
// consume, u8 bins[F, N], made from the uploaded f32 matrix x[N, F].
//
// bin_select summarises a group of at most BIN_GROUP_COLS columns with a
// multi-rank radix select over order-preserving u32 keys (-0.0 and +0.0 share
// one key), four 8-bit digit passes from the top:
//
//   bin_keys_kernel   x row-major -> keys[G, N] column-major through a
//                     64 x 64 LDS tile, both sides coalesced (the one extra
//                     copy of the block);
//   bin_count_kernel  hist[column][slot][digit] += 1 for every row whose key
//                     prefix is one of the column's active prefixes (slots);
//   bin_plan_kernel   one block per column turns the counts into the next
//                     pass's slot table.
//
// A column's state is BIN_ST_WORDS i64 words: {slots, mode, prefix[256],
// base[256]}; base is the rank of the slot's first key in the sorted column.
// While a column's non-empty buckets number <= max_bins (mode 0) all of them
// stay active, and after the last pass they are its distinct values. Once
// they exceed max_bins the column is a quantile column for good (mode 1):
// only buckets that hold one of the ranks (k * N) / max_bins, k = 1 ..
// max_bins - 1, or the last rank N - 1 (the maximum) stay, at most max_bins
// of them. Counters are integers and accumulate across launches over row
// slices, so the result does not depend on the order atomics land in.
//
// bin_assign_kernel stages a column's edge keys in LDS and writes
// bins[f][r] = #{edges < x} by binary search over them, from the
// column-major keys: reads and byte writes are both coalesced.
//
// No kernel here computes in floating point: x is read as its bit pattern.
// ---------------------------------------------------------------------------

#define BIN_BLOCK 256
#define BIN_SLOTS 256          // most active prefixes of a column (HGBT_MAX_BINS)
#define BIN_DIGITS 256         // 8-bit digits, four passes
#define BIN_LDS_SLOTS 60       // counters live in LDS up to this many slots (60 KiB)
#define BIN_ROWS_PER_BLOCK 16384
#define BIN_GROUP_COLS 64      // columns of one bin_select call (16 MiB of counters)
#define BIN_TILE 64
#define BIN_AGG_ROUNDS 4       // same-address rounds of a wave before plain atomics
#define BIN_ST_WORDS (2 + 2 * BIN_SLOTS)
static_assert(BIN_SLOTS == HGBT_MAX_BINS && BIN_SLOTS <= BIN_BLOCK,
              "one thread per slot stages a column's table");
static_assert(BIN_DIGITS == BIN_BLOCK, "bin_plan_kernel: one thread per digit");
static_assert((BIN_LDS_SLOTS * BIN_DIGITS + BIN_SLOTS) * 4 <= 64 * 1024,
              "static LDS of bin_count_kernel; two blocks per CU");

#if defined(__HIP_DEVICE_COMPILE__)
#define BIN_NO_PACKED_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define BIN_NO_PACKED_F32
#endif

// Order-preserving key of a finite f32 bit pattern; both zeros give 0x80000000.
__device__ __forceinline__ unsigned bin_key(unsigned u) {
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// grid = (64-row tiles of the slice [r0, r1), 64-column tiles of the group).
BIN_NO_PACKED_F32
__global__ __launch_bounds__(BIN_BLOCK) void bin_keys_kernel(
    const unsigned* __restrict__ x, long long n_rows, int n_feat, int f0, int g_cols,
    long long r0, long long r1, unsigned* __restrict__ keys)
{
  __shared__ unsigned tile[BIN_TILE][BIN_TILE + 1];
  const int tx = threadIdx.x & (BIN_TILE - 1), ty = threadIdx.x / BIN_TILE;
  const long long rb = r0 + (long long)blockIdx.x * BIN_TILE;
  const int cb = (int)blockIdx.y * BIN_TILE;
  for (int i = ty; i < BIN_TILE; i += BIN_BLOCK / BIN_TILE) {
    const long long r = rb + i;
    const int c = cb + tx;
    if (r < r1 && c < g_cols)
      tile[i][tx] = bin_key(x[(size_t)r * (size_t)n_feat + (size_t)(f0 + c)]);
  }
  __syncthreads();
  for (int i = ty; i < BIN_TILE; i += BIN_BLOCK / BIN_TILE) {
    const int c = cb + i;
    const long long r = rb + tx;
    if (c < g_cols && r < r1) keys[(size_t)c * (size_t)n_rows + (size_t)r] = tile[tx][i];
  }
}

// One counter increment per lane (idx < 0: none) with same-address
// aggregation: for up to BIN_AGG_ROUNDS rounds the first pending lane's
// address is broadcast and every lane holding it retires through one atomic
// of the group's size; what is left goes on its own. A column of mostly one
// value costs one atomic per wave instead of 64 on one address. Every lane of
// the wave must call this.
__device__ __forceinline__ void bin_wave_add(unsigned* __restrict__ cnt, int idx) {
  const int lane = threadIdx.x & 63;
  bool pending = idx >= 0;
  for (int round = 0; round < BIN_AGG_ROUNDS; ++round) {
    const unsigned long long act = __ballot(pending);
    if (!act) return;
    const int leader = __ffsll((long long)act) - 1;
    const int lidx = __shfl(idx, leader);
    const bool same = pending && idx == lidx;
    const unsigned long long grp = __ballot(same);
    if (same) {
      if (lane == leader) atomicAdd(cnt + lidx, (unsigned)__popcll(grp));
      pending = false;
    }
  }
  if (pending) atomicAdd(cnt + idx, 1u);
}

// grid = (row blocks of the slice [r0, r1), columns of the group). Digit pass
// with the digit at bit `shift` (24, 16, 8, 0); the prefix is the key above
// it. hist is u32[g_cols, BIN_SLOTS, BIN_DIGITS]. Up to BIN_LDS_SLOTS slots
// the block counts in LDS and flushes its non-zero counters; above, it counts
// straight into hist. Slot indices come from a bounded search over the
// clamped table, so no table content can index outside hist.
BIN_NO_PACKED_F32
__global__ __launch_bounds__(BIN_BLOCK) void bin_count_kernel(
    const unsigned* __restrict__ keys, long long n_rows, long long r0, long long r1,
    int g_cols, int shift, const long long* __restrict__ st,
    unsigned* __restrict__ hist)
{
  __shared__ unsigned s_prefix[BIN_SLOTS];
  __shared__ unsigned s_cnt[BIN_LDS_SLOTS * BIN_DIGITS];
  const int c = blockIdx.y, tid = threadIdx.x;
  if (c >= g_cols) return;
  const long long* cst = st + (size_t)c * BIN_ST_WORDS;
  const int ns = (int)min(max(cst[0], 0ll), (long long)BIN_SLOTS);
  if (ns == 0) return;
  const bool use_lds = ns <= BIN_LDS_SLOTS;
  if (tid < ns) s_prefix[tid] = (unsigned)cst[2 + tid];
  if (use_lds)
    for (int i = tid; i < ns * BIN_DIGITS; i += BIN_BLOCK) s_cnt[i] = 0u;
  __syncthreads();

  const unsigned* col = keys + (size_t)c * (size_t)n_rows;
  unsigned* gh = hist + (size_t)c * BIN_SLOTS * BIN_DIGITS;
  const long long b0 = r0 + (long long)blockIdx.x * BIN_ROWS_PER_BLOCK;
  const long long b1 = min(b0 + (long long)BIN_ROWS_PER_BLOCK, r1);
  // the trip count is the block's: whole waves reach bin_wave_add
  for (long long rr = b0; rr < b1; rr += BIN_BLOCK) {
    const long long r = rr + tid;
    int idx = -1;
    if (r < b1) {
      const unsigned k = col[r];
      const unsigned pre = (shift >= 24) ? 0u : (k >> (shift + 8));
      int lo = 0, hi = ns;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_prefix[mid] < pre) lo = mid + 1; else hi = mid;
      }
      if (lo < ns && s_prefix[lo] == pre)
        idx = lo * BIN_DIGITS + (int)((k >> shift) & (BIN_DIGITS - 1));
    }
    if (use_lds) {
      if (idx >= 0) atomicAdd(&s_cnt[idx], 1u);
    } else {
      bin_wave_add(gh, idx);
    }
  }
  if (use_lds) {
    __syncthreads();
    for (int i = tid; i < ns * BIN_DIGITS; i += BIN_BLOCK) {
      const unsigned v = s_cnt[i];
      if (v) atomicAdd(gh + i, v);
    }
  }
}

// Exclusive prefix sum of v over the block's 256 threads and its total.
__device__ __forceinline__ void bin_block_scan(
    unsigned v, unsigned* s_wave, unsigned& excl, unsigned& total)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned inc = v;
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned t = __shfl_up(inc, d);
    if (lane >= d) inc += t;
  }
  __syncthreads();  // the previous scan's readers are done with s_wave
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  unsigned before = 0, tot = 0;
  for (int w = 0; w < BIN_BLOCK / 64; ++w) {
    const unsigned t = s_wave[w];
    if (w < wave) before += t;
    tot += t;
  }
  excl = before + inc - v;
  total = tot;
}

// #{k in 1 .. max_bins-1 : (k * n) / max_bins < x} for 0 <= x <= n, in int64.
__device__ __forceinline__ long long bin_ranks_below(long long x, long long n, int max_bins) {
  const long long k = (x * max_bins + n - 1) / n - 1;
  return min(max(k, 0ll), (long long)(max_bins - 1));
}

// grid = columns of the group; thread = digit. Walks the column's slots in
// key order; bucket (slot, digit) starts at rank base[slot] + the counts of
// the slot's lower digits. Kept buckets become the next table, compacted in
// order; at most BIN_SLOTS are written.
BIN_NO_PACKED_F32
__global__ __launch_bounds__(BIN_BLOCK) void bin_plan_kernel(
    const unsigned* __restrict__ hist, int g_cols, long long n_total, int max_bins,
    long long* __restrict__ st)
{
  __shared__ unsigned s_prefix[BIN_SLOTS];
  __shared__ long long s_base[BIN_SLOTS];
  __shared__ unsigned s_wave[BIN_BLOCK / 64];
  __shared__ int s_nonempty;
  const int c = blockIdx.x, tid = threadIdx.x;
  if (c >= g_cols) return;
  long long* cst = st + (size_t)c * BIN_ST_WORDS;
  const int ns = (int)min(max(cst[0], 0ll), (long long)BIN_SLOTS);
  int mode = cst[1] != 0;
  if (tid < ns) {
    s_prefix[tid] = (unsigned)cst[2 + tid];
    s_base[tid] = cst[2 + BIN_SLOTS + tid];
  }
  if (tid == 0) s_nonempty = 0;
  __syncthreads();
  const unsigned* h = hist + (size_t)c * BIN_SLOTS * BIN_DIGITS;
  if (mode == 0) {
    int mine = 0;
    for (int s = 0; s < ns; ++s) mine += h[s * BIN_DIGITS + tid] != 0u;
    if (mine) atomicAdd(&s_nonempty, mine);
    __syncthreads();
    if (s_nonempty > max_bins) mode = 1;
  }
  int out = 0;
  for (int s = 0; s < ns; ++s) {
    const unsigned cnt = h[s * BIN_DIGITS + tid];
    unsigned below, slot_total;
    bin_block_scan(cnt, s_wave, below, slot_total);
    const long long b = s_base[s] + (long long)below, e = b + (long long)cnt;
    bool keep = cnt != 0u;
    if (keep && mode == 1)
      keep = e == n_total ||
             bin_ranks_below(e, n_total, max_bins) > bin_ranks_below(b, n_total, max_bins);
    unsigned pos, kept;
    bin_block_scan(keep ? 1u : 0u, s_wave, pos, kept);
    const int at = out + (int)pos;
    if (keep && at < BIN_SLOTS) {
      cst[2 + at] = (long long)((s_prefix[s] << 8) | (unsigned)tid);
      cst[2 + BIN_SLOTS + at] = b;
    }
    out += (int)kept;
  }
  if (tid == 0) {
    cst[0] = min(out, BIN_SLOTS);
    cst[1] = mode;
  }
}

// grid = (row blocks of the slice [r0, r1), columns of the group). edges is
// i32[g_cols, BIN_SLOTS]: the column's edge count, then its ascending edge
// keys. bins points at the group's first row of the u8[F, N] matrix.
BIN_NO_PACKED_F32
__global__ __launch_bounds__(BIN_BLOCK) void bin_assign_kernel(
    const unsigned* __restrict__ keys, long long n_rows, long long r0, long long r1,
    int g_cols, const int* __restrict__ edges, uint8_t* __restrict__ bins)
{
  __shared__ unsigned s_edge[BIN_SLOTS];
  const int c = blockIdx.y, tid = threadIdx.x;
  if (c >= g_cols) return;
  const int ne = min(max(edges[(size_t)c * BIN_SLOTS], 0), BIN_SLOTS - 1);
  if (tid < ne) s_edge[tid] = (unsigned)edges[(size_t)c * BIN_SLOTS + 1 + tid];
  __syncthreads();
  const unsigned* col = keys + (size_t)c * (size_t)n_rows;
  uint8_t* out = bins + (size_t)c * (size_t)n_rows;
  const long long b0 = r0 + (long long)blockIdx.x * BIN_ROWS_PER_BLOCK;
  const long long b1 = min(b0 + (long long)BIN_ROWS_PER_BLOCK, r1);
  for (long long r = b0 + tid; r < b1; r += BIN_BLOCK) {
    const unsigned k = col[r];
    int lo = 0, hi = ne;  // #{edges < key}
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s_edge[mid] < k) lo = mid + 1; else hi = mid;
    }
    out[r] = (uint8_t)lo;
  }
}

// Summary of the columns [f0, f1) of x f32[N, F]: {keys i32[G, N] (the u32
// keys, column-major), st i64[G, BIN_ST_WORDS]}. After the four passes a
// column's slots are whole keys: its distinct values in mode 0; in mode 1 the
// values that hold the quantile ranks and the maximum, each with the rank of
// its first occurrence. No launch covers more than launch_rows rows.
std::vector<torch::Tensor> bin_select(
    torch::Tensor x, int64_t f0, int64_t f1, int64_t max_bins, int64_t launch_rows)
{
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == torch::kFloat32 && x.dim() == 2 &&
              x.is_contiguous(), "x must be a contiguous f32[N, F] GPU tensor");
  const int64_t N = x.size(0), F = x.size(1);
  TORCH_CHECK(N >= 1 && N < (int64_t(1) << 31), "row count out of range (u32 counters)");
  TORCH_CHECK(F >= 1 && F < (int64_t(1) << 31), "feature count out of range");
  TORCH_CHECK(0 <= f0 && f0 < f1 && f1 <= F && f1 - f0 <= BIN_GROUP_COLS,
              "a column group is [f0, f1) with at most ", BIN_GROUP_COLS, " columns");
  TORCH_CHECK(max_bins >= 2 && max_bins <= HGBT_MAX_BINS, "max_bins must be in [2, 256]");
  TORCH_CHECK(launch_rows >= 1, "launch_rows must be >= 1");
  const int64_t G = f1 - f0;
  c10::hip::HIPGuard guard((c10::DeviceIndex)x.get_device());
  const auto i32 = torch::TensorOptions().dtype(torch::kInt32).device(x.device());
  auto keys = torch::empty({G, N}, i32);
  auto hist = torch::empty({G, BIN_SLOTS, BIN_DIGITS}, i32);
  auto st = torch::zeros({G, BIN_ST_WORDS}, i32.dtype(torch::kInt64));
  st.select(1, 0).fill_(1);  // one slot: the empty prefix, base rank 0, mode 0
  hipStream_t stream = c10::hip::getCurrentHIPStream();
  unsigned* kp = reinterpret_cast<unsigned*>(keys.data_ptr<int>());
  unsigned* hp = reinterpret_cast<unsigned*>(hist.data_ptr<int>());
  long long* sp = reinterpret_cast<long long*>(st.data_ptr<int64_t>());
  const int col_tiles = (int)((G + BIN_TILE - 1) / BIN_TILE);
  for (int64_t a = 0; a < N; a += launch_rows) {
    const int64_t b = std::min(N, a + launch_rows);
    hipLaunchKernelGGL(bin_keys_kernel,
        dim3((unsigned)((b - a + BIN_TILE - 1) / BIN_TILE), (unsigned)col_tiles),
        dim3(BIN_BLOCK), 0, stream,
        reinterpret_cast<const unsigned*>(x.data_ptr<float>()), (long long)N, (int)F,
        (int)f0, (int)G, (long long)a, (long long)b, kp);
    HIP_CHECK(hipGetLastError());
  }
  for (int shift = 24; shift >= 0; shift -= 8) {
    hist.zero_();
    for (int64_t a = 0; a < N; a += launch_rows) {
      const int64_t b = std::min(N, a + launch_rows);
      hipLaunchKernelGGL(bin_count_kernel,
          dim3((unsigned)((b - a + BIN_ROWS_PER_BLOCK - 1) / BIN_ROWS_PER_BLOCK), (unsigned)G),
          dim3(BIN_BLOCK), 0, stream,
          kp, (long long)N, (long long)a, (long long)b, (int)G, shift, sp, hp);
      HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(bin_plan_kernel, dim3((unsigned)G), dim3(BIN_BLOCK), 0, stream,
        hp, (int)G, (long long)N, (int)max_bins, sp);
    HIP_CHECK(hipGetLastError());
  }
  return {keys, st};
}

// bins[f0 + c][r] = #{edges of column c < key} for the group whose keys
// bin_select returned; edges i32[G, BIN_SLOTS] = {count, edge keys ...}.
void bin_assign(torch::Tensor keys, torch::Tensor edges, torch::Tensor bins,
                int64_t f0, int64_t launch_rows)
{
  TORCH_CHECK(bins.is_cuda() && bins.scalar_type() == torch::kUInt8 &&
              bins.dim() == 2 && bins.is_contiguous(),
              "bins must be a contiguous u8[F, N] GPU tensor");
  hgbt_check(keys, bins, torch::kInt32, "keys");
  hgbt_check(edges, bins, torch::kInt32, "edges");
  const int64_t N = bins.size(1);
  TORCH_CHECK(keys.dim() == 2 && keys.size(1) == N && keys.size(0) >= 1,
              "keys must be i32[G, N]");
  const int64_t G = keys.size(0);
  TORCH_CHECK(edges.dim() == 2 && edges.size(0) == G && edges.size(1) == BIN_SLOTS,
              "edges must be i32[G, ", BIN_SLOTS, "]");
  TORCH_CHECK(f0 >= 0 && f0 + G <= bins.size(0), "column group outside the bin matrix");
  TORCH_CHECK(launch_rows >= 1, "launch_rows must be >= 1");
  if (N == 0) return;
  c10::hip::HIPGuard guard((c10::DeviceIndex)bins.get_device());
  hipStream_t stream = c10::hip::getCurrentHIPStream();
  for (int64_t a = 0; a < N; a += launch_rows) {
    const int64_t b = std::min(N, a + launch_rows);
    hipLaunchKernelGGL(bin_assign_kernel,
        dim3((unsigned)((b - a + BIN_ROWS_PER_BLOCK - 1) / BIN_ROWS_PER_BLOCK), (unsigned)G),
        dim3(BIN_BLOCK), 0, stream,
        reinterpret_cast<const unsigned*>(keys.data_ptr<int>()), (long long)N,
        (long long)a, (long long)b, (int)G, edges.data_ptr<int>(),
        bins.data_ptr<uint8_t>() + (size_t)f0 * (size_t)N);
    HIP_CHECK(hipGetLastError());
  }
}

// ---------------------------------------------------------------------------
// Histogram random-forest trainer (creditcore/models/hrf.py).
//
// A forest's trees are independent, so a batch of TB trees grows in the same
// launches: one level of the whole batch = hrf_hist_kernel, hrf_split_kernel,
// hrf_route_kernel and one copy of the split records to the host. The level
// is a flat list of open slots; slot_off i32[TB+1] gives each tree's range in
// it and slot_meta i32[K, 2] = (global tree index, node id) per slot.
//
// Layouts: bins u8[F, N] and y u8[N] (0/1) are shared by the batch; w u8[TB, N]
// are the bootstrap counts and node i32[TB, N] the row's local slot within
// its tree (negative: in a leaf, or weight 0). Histogram i64[K, 2, total_bins]
// with planes {sum w*y, sum w}: integers, so order independent, and the CPU
// reference (ops/cpu_ref.py hrf_*_cpu) must match bit for bit.
// ---------------------------------------------------------------------------

#define HRF_REC 7  // split record, i64 words: proxy bits, feat, bin, PL, WL, P, W
#define HRF_MAX_FEATS 1024  // per-feature LDS tables of hrf_split_kernel
// odd multipliers of the feature key (cpu_ref.HRF_C1..3)
#define HRF_C1 0x9E3779B97F4A7C15ull
#define HRF_C2 0xC2B2AE3D27D4EB4Full
#define HRF_C3 0x165667B19E3779F9ull
// A block's int32 LDS partial is at most rows_per_block * 255. The cap is far
// below that bound on purpose: 32 rows per thread keep the slab flush a small
// share of a block's work while (row blocks x groups x trees) still fills the
// chip at a few thousand rows.
static constexpr int64_t HRF_MAX_ROWS_PER_BLOCK = 32 * HGBT_BLOCK;
static_assert(HRF_MAX_ROWS_PER_BLOCK * 255 < (int64_t(1) << 31),
              "int32 LDS partials of hrf_hist_kernel would overflow");

// grid = (row blocks, feature groups, tree in batch). lds_entries > 0: the
// block's (open slots of its tree x 2 x group bins) slab is summed in LDS and
// flushed with one global atomic per non-zero entry; lds_entries == 0: int64
// atomics straight to global memory. Offsets read from slot_off / bin_off /
// grp_off are range-checked before use: bad contents skip work.
__global__ __launch_bounds__(HGBT_BLOCK) void hrf_hist_kernel(
    const uint8_t* __restrict__ bins, const int* __restrict__ bin_off,
    const int* __restrict__ grp_off, const uint8_t* __restrict__ y,
    const uint8_t* __restrict__ w, const int* __restrict__ node,
    const int* __restrict__ slot_off,
    long long n_rows, int n_feat, int n_slots, int total_bins,
    int rows_per_block, int lds_entries,
    unsigned long long* __restrict__ hist)
{
  extern __shared__ int hrf_lds[];
  const int tid = threadIdx.x;
  const int t = blockIdx.z;
  const int s0 = slot_off[t];
  const int k = slot_off[t + 1] - s0;  // open slots of this tree
  if (s0 < 0 || k <= 0 || (long long)s0 + k > n_slots) return;
  const int f0 = grp_off[blockIdx.y], f1 = grp_off[blockIdx.y + 1];
  if (f0 < 0 || f1 > n_feat || f0 >= f1) return;
  const int b0 = bin_off[f0];
  const int gb = bin_off[f1] - b0;  // bins of this feature group
  if (b0 < 0 || gb <= 0 || (long long)b0 + gb > total_bins) return;
  const bool use_lds = lds_entries > 0;
  const long long slab = (long long)k * 2 * gb;
  if (use_lds) {
    if (slab > lds_entries) return;  // host sizes the allocation from the same tables
    for (int i = tid; i < (int)slab; i += HGBT_BLOCK) hrf_lds[i] = 0;
    __syncthreads();
  }
  unsigned long long* thist = hist + (size_t)s0 * 2 * total_bins;
  const uint8_t* tw = w + (size_t)t * (size_t)n_rows;
  const int* tnode = node + (size_t)t * (size_t)n_rows;

  const long long r0 = (long long)blockIdx.x * rows_per_block;
  const long long r1 = min(r0 + (long long)rows_per_block, n_rows);
  for (long long r = r0 + tid; r < r1; r += HGBT_BLOCK) {
    const int nd = tnode[r];
    if (nd < 0 || nd >= k) continue;  // in a leaf, or out of the bootstrap
    const int wt = tw[r];
    if (wt == 0) continue;
    const int wy = y[r] ? wt : 0;
    for (int f = f0; f < f1; ++f) {
      const int fb = bin_off[f];
      const int nb = bin_off[f + 1] - fb;
      if (fb < b0 || nb <= 0 || fb + nb > b0 + gb) continue;
      const int b = bins[(size_t)f * (size_t)n_rows + (size_t)r];
      if (b >= nb) continue;
      if (use_lds) {
        int* p = hrf_lds + (size_t)nd * 2 * gb + (fb - b0) + b;
        if (wy) atomicAdd(p, wy);
        atomicAdd(p + gb, wt);
      } else {
        unsigned long long* p = thist + (size_t)nd * 2 * total_bins + fb + b;
        if (wy) atomicAdd(p, (unsigned long long)wy);
        atomicAdd(p + total_bins, (unsigned long long)wt);
      }
    }
  }

  if (use_lds) {
    __syncthreads();
    for (int i = tid; i < (int)slab; i += HGBT_BLOCK) {
      const int v = hrf_lds[i];
      if (v == 0) continue;
      const int plane = i / gb;  // local slot * 2 + {w*y, w}
      const int b = i - plane * gb;
      atomicAdd(thist + (size_t)plane * total_bins + b0 + b, (unsigned long long)v);
    }
  }
}

// Gini proxy PL^2/WL + PR^2/WR - P^2/W from the integer sums, in f64. The
// operation order is hrf_split_cpu's and contraction is off (see hgbt_gain).
__device__ __forceinline__ double hrf_proxy(
    long long PL, long long WL, long long P, long long W)
{
#pragma clang fp contract(off)
  const double pl = (double)PL, wl = (double)WL;
  const double pr = (double)(P - PL), wr = (double)(W - WL);
  const double p = (double)P, w = (double)W;
  const double a = (pl * pl) / wl;
  const double b = (pr * pr) / wr;
  const double c = (p * p) / w;
  return (a + b) - c;
}

__device__ __forceinline__ unsigned long long hrf_key(
    unsigned long long seed, int tree, int node_id, int f)
{
  // int -> i64 -> u64, as cpu_ref.hrf_feature_keys converts
  unsigned long long z = seed ^ ((unsigned long long)(long long)tree * HRF_C1)
                              ^ ((unsigned long long)(long long)node_id * HRF_C2)
                              ^ ((unsigned long long)f * HRF_C3);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

struct HrfPick {
  double proxy;
  int rank, feat;  // rank < 0 = nothing picked yet
};

// highest proxy, then the lower rank
__device__ __forceinline__ bool hrf_better(const HrfPick& a, const HrfPick& b) {
  if (a.rank < 0) return false;
  if (b.rank < 0) return true;
  if (a.proxy != b.proxy) return a.proxy > b.proxy;
  return a.rank < b.rank;
}

// LDS tables of one slot's split choice, one entry per feature (bin -1: the
// feature has no valid split). hrf_split_kernel and hrf_seg_split_kernel fill
// them in phase 1 and hand them to hrf_pick_split.
struct HrfTables {
  double* proxy;
  unsigned long long* key;
  long long *pl, *wl;
  int *bin, *rank;
  long long* tot;  // [2]: the slot's P and W
  int* r_star;
  HrfPick* wave_pick;  // [HGBT_BLOCK / 64]
};

// Phase 1 for one feature, by one wavefront (hgbt_split_kernel's scan): hp /
// hw are the feature's nb bins of the two planes, a lane owns 4 of them, and
// the feature's best valid split (highest proxy, lowest bin) goes to the
// tables. nb <= 0 records "no valid split". T is the histogram's word: i64
// in global memory (hrf_split_kernel) or i32 in LDS (hrf_seg_split_kernel).
template <typename T>
__device__ __forceinline__ void hrf_scan_feature(
    const T* hp, const T* hw, int nb, int f, int lane, long long min_leaf,
    const HrfTables& t)
{
  double bp = 0.0;
  int bb = -1;
  long long bpl = 0, bwl = 0;
  if (nb > 0) {
    long long pp[4], pw[4];
    long long sp = 0, sw = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int b = lane * 4 + j;
      if (b < nb) { sp += hp[b]; sw += hw[b]; }
      pp[j] = sp; pw[j] = sw;
    }
    long long ip = sp, iw = sw;  // inclusive scan of the lane totals
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long tp = __shfl_up(ip, d), tw = __shfl_up(iw, d);
      if (lane >= d) { ip += tp; iw += tw; }
    }
    const long long P = __shfl(ip, 63), W = __shfl(iw, 63);
    // every feature sees every open row once: feature 0's totals are the slot's
    if (f == 0 && lane == 0) { t.tot[0] = P; t.tot[1] = W; }
    const long long op = ip - sp, ow = iw - sw;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int b = lane * 4 + j;
      if (b >= nb) continue;
      const long long WL = ow + pw[j], PL = op + pp[j];
      if (WL < min_leaf || W - WL < min_leaf) continue;
      const double px = hrf_proxy(PL, WL, P, W);
      if (!(px > 0.0)) continue;
      if (bb < 0 || px > bp) { bp = px; bb = b; bpl = PL; bwl = WL; }  // ascending b
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const double op_ = __shfl_xor(bp, m);
      const int ob = __shfl_xor(bb, m);
      const long long opl = __shfl_xor(bpl, m), owl = __shfl_xor(bwl, m);
      const bool take = ob >= 0 && (bb < 0 || op_ > bp || (op_ == bp && ob < bb));
      if (take) { bp = op_; bb = ob; bpl = opl; bwl = owl; }
    }
  }
  if (lane == 0) { t.proxy[f] = bp; t.bin[f] = bb; t.pl[f] = bpl; t.wl[f] = bwl; }
}

// Phase 2, by the whole block once every feature's entry is written (it
// starts with the barrier that makes them visible): feature keys, ranks by
// (key, f), r* = lowest rank with a valid split, and among the ranks below
// max(max_features, r* + 1) the highest proxy, ties to the lower rank. Thread
// 0 writes the slot's record. *t.r_star must hold n_feat on entry.
__device__ __forceinline__ void hrf_pick_split(
    const HrfTables& t, int n_feat, int max_features, unsigned long long seed,
    int tree, int node_id, long long* __restrict__ o)
{
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  for (int f = tid; f < n_feat; f += HGBT_BLOCK) t.key[f] = hrf_key(seed, tree, node_id, f);
  __syncthreads();

  for (int f = tid; f < n_feat; f += HGBT_BLOCK) {
    const unsigned long long kf = t.key[f];
    int rank = 0;
    for (int g = 0; g < n_feat; ++g) {  // same g across the wave: LDS broadcast
      const unsigned long long kg = t.key[g];
      rank += (kg < kf || (kg == kf && g < f)) ? 1 : 0;
    }
    t.rank[f] = rank;
    if (t.bin[f] >= 0) atomicMin(t.r_star, rank);
  }
  __syncthreads();

  const int limit = max(max_features, *t.r_star + 1);
  HrfPick best;
  best.proxy = 0.0; best.rank = -1; best.feat = -1;
  for (int f = tid; f < n_feat; f += HGBT_BLOCK) {
    if (t.bin[f] < 0 || t.rank[f] >= limit) continue;
    HrfPick c;
    c.proxy = t.proxy[f]; c.rank = t.rank[f]; c.feat = f;
    if (hrf_better(c, best)) best = c;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    HrfPick o2;
    o2.proxy = __shfl_xor(best.proxy, m);
    o2.rank = __shfl_xor(best.rank, m);
    o2.feat = __shfl_xor(best.feat, m);
    if (hrf_better(o2, best)) best = o2;
  }
  if (lane == 0) t.wave_pick[wave] = best;
  __syncthreads();
  if (tid == 0) {
    for (int wv = 1; wv < HGBT_BLOCK / 64; ++wv)
      if (hrf_better(t.wave_pick[wv], best)) best = t.wave_pick[wv];
    const bool ok = best.rank >= 0;
    o[0] = __double_as_longlong(ok ? best.proxy : 0.0);
    o[1] = ok ? best.feat : -1;
    o[2] = ok ? t.bin[best.feat] : 0;
    o[3] = ok ? t.pl[best.feat] : 0;
    o[4] = ok ? t.wl[best.feat] : 0;
    o[5] = t.tot[0]; o[6] = t.tot[1];
  }
}

// One block per open slot over the level's dense histogram. Phase 1: each
// wavefront takes every 4th feature (hrf_scan_feature); phase 2:
// hrf_pick_split.
__global__ __launch_bounds__(HGBT_BLOCK) void hrf_split_kernel(
    const long long* __restrict__ hist, const int* __restrict__ bin_off,
    const int* __restrict__ slot_meta, int n_feat, int total_bins,
    int max_features, long long min_leaf, unsigned long long seed,
    long long* __restrict__ out)
{
  __shared__ double f_proxy[HRF_MAX_FEATS];
  __shared__ unsigned long long f_key[HRF_MAX_FEATS];
  __shared__ long long f_pl[HRF_MAX_FEATS], f_wl[HRF_MAX_FEATS];
  __shared__ int f_bin[HRF_MAX_FEATS];
  __shared__ int f_rank[HRF_MAX_FEATS];
  __shared__ long long tot[2];
  __shared__ int r_star;
  __shared__ HrfPick wave_pick[HGBT_BLOCK / 64];
  const HrfTables t = {f_proxy, f_key, f_pl, f_wl, f_bin, f_rank, tot, &r_star, wave_pick};
  const int k = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const long long* hp = hist + (size_t)k * 2 * total_bins;
  const long long* hw = hp + total_bins;
  if (n_feat > HRF_MAX_FEATS) return;  // the wrapper refuses this too

  if (tid == 0) { r_star = n_feat; tot[0] = tot[1] = 0; }
  for (int f = wave; f < n_feat; f += HGBT_BLOCK / 64) {
    const int fb = bin_off[f];
    const int nb = bin_off[f + 1] - fb;
    const bool ok = !(fb < 0 || nb <= 0 || nb > HGBT_MAX_BINS || fb + nb > total_bins);
    hrf_scan_feature(ok ? hp + fb : hp, ok ? hw + fb : hw, ok ? nb : 0, f, lane, min_leaf, t);
  }
  hrf_pick_split(t, n_feat, max_features, seed, slot_meta[2 * k], slot_meta[2 * k + 1],
                 out + (size_t)k * HRF_REC);
}

// grid = (row blocks, tree). hgbt_route_kernel's table protocol with the
// table indexed by slot_off[t] + local slot; targets are local slots of the
// tree's next level or -(leaf node + 1).
__global__ __launch_bounds__(HGBT_BLOCK) void hrf_route_kernel(
    const uint8_t* __restrict__ bins, const int4* __restrict__ table,
    const int* __restrict__ slot_off, long long n_rows, int n_feat, int n_slots,
    int* __restrict__ node)
{
  const long long r = (long long)blockIdx.x * HGBT_BLOCK + threadIdx.x;
  if (r >= n_rows) return;
  const int t = blockIdx.y;
  const int s0 = slot_off[t];
  const int k = slot_off[t + 1] - s0;
  if (s0 < 0 || k <= 0 || (long long)s0 + k > n_slots) return;
  int* tnode = node + (size_t)t * (size_t)n_rows;
  const int nd = tnode[r];
  if (nd < 0 || nd >= k) return;
  const int4 e = table[s0 + nd];
  if (e.x < 0) {
    tnode[r] = e.z;
  } else if (e.x < n_feat) {
    const int b = bins[(size_t)e.x * (size_t)n_rows + (size_t)r];
    tnode[r] = (b <= e.y) ? e.z : e.w;
  }
}

// ---------------------------------------------------------------------------
// Segmented levels (HistForestClassifier(deep_trees=True), levels from
// _dense_levels on). A deep level has many slots of a few rows each, so its
// dense histogram would be gigabytes of zeros. Instead the level's open rows
// are bucketed by slot,
//
//   hrf_seg_count_kernel    rows per slot            -> cnt i32[K]
//   hrf_seg_scan_kernel     exclusive scan           -> seg_off i32[K+1]
//   hrf_seg_scatter_kernel  per-slot atomic cursors  -> rows int2[open rows]
//
// and hrf_seg_split_kernel builds each slot's histogram in LDS, one feature
// per wavefront at a time, and scans it on the spot: memory is O(open rows +
// K). A rows entry is {row id, w | y << 8}; the order inside a segment is
// whatever the atomics gave, which cannot show in a record because every sum
// is an integer. The records equal hrf_split_kernel's over hrf_hist_kernel's
// histogram bit for bit.
// ---------------------------------------------------------------------------

#define HRF_SEG_CHUNK 512    // rows of a slot staged in LDS per pass
#define HRF_SCAN_BLOCK 1024  // hrf_seg_scan_kernel's only block

// Flat slot of row r of tree t, or -1: in a leaf, weight 0, or bad offsets.
__device__ __forceinline__ int hrf_open_slot(
    const int* __restrict__ slot_off, const int* __restrict__ node,
    const uint8_t* __restrict__ w, long long n_rows, int n_slots, int t, long long r)
{
  const int s0 = slot_off[t];
  const int k = slot_off[t + 1] - s0;
  if (s0 < 0 || k <= 0 || (long long)s0 + k > n_slots) return -1;
  const size_t at = (size_t)t * (size_t)n_rows + (size_t)r;
  const int nd = node[at];
  if (nd < 0 || nd >= k || w[at] == 0) return -1;
  return s0 + nd;
}

// grid = (row blocks, tree). cnt must be zero on entry.
__global__ __launch_bounds__(HGBT_BLOCK) void hrf_seg_count_kernel(
    const uint8_t* __restrict__ w, const int* __restrict__ node,
    const int* __restrict__ slot_off, long long n_rows, int n_slots,
    int* __restrict__ cnt)
{
  const long long r = (long long)blockIdx.x * HGBT_BLOCK + threadIdx.x;
  if (r >= n_rows) return;
  const int s = hrf_open_slot(slot_off, node, w, n_rows, n_slots, blockIdx.y, r);
  if (s >= 0) atomicAdd(cnt + s, 1);
}

// One block: seg_off[i] = sum of cnt[0..i), seg_off[n_slots] = the total. The
// block walks cnt in HRF_SCAN_BLOCK pieces and carries the running total.
__global__ __launch_bounds__(HRF_SCAN_BLOCK) void hrf_seg_scan_kernel(
    const int* __restrict__ cnt, int n_slots, int* __restrict__ seg_off)
{
  __shared__ int wave_sum[HRF_SCAN_BLOCK / 64];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  int carry = 0;
  for (int base = 0; base < n_slots; base += HRF_SCAN_BLOCK) {
    const int i = base + tid;
    const int v = i < n_slots ? cnt[i] : 0;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(inc, d);
      if (lane >= d) inc += o;
    }
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int j = 0; j < HRF_SCAN_BLOCK / 64; ++j) {
      const int ws = wave_sum[j];
      if (j < wave) before += ws;
      total += ws;
    }
    if (i < n_slots) seg_off[i] = carry + before + inc - v;
    carry += total;
    __syncthreads();  // wave_sum is rewritten by the next piece
  }
  if (tid == 0) seg_off[n_slots] = carry;
}

// grid = (row blocks, tree). cursor must be zero on entry. A row that does
// not fit its segment or the rows array (contents changed since the count,
// or max_open too small) is dropped, never written out of range.
__global__ __launch_bounds__(HGBT_BLOCK) void hrf_seg_scatter_kernel(
    const uint8_t* __restrict__ w, const uint8_t* __restrict__ y,
    const int* __restrict__ node, const int* __restrict__ slot_off,
    const int* __restrict__ seg_off, long long n_rows, int n_slots, int max_open,
    int* __restrict__ cursor, int2* __restrict__ rows)
{
  const long long r = (long long)blockIdx.x * HGBT_BLOCK + threadIdx.x;
  if (r >= n_rows) return;
  const int t = blockIdx.y;
  const int s = hrf_open_slot(slot_off, node, w, n_rows, n_slots, t, r);
  if (s < 0) return;
  const int a = seg_off[s];
  const int len = seg_off[s + 1] - a;
  const int pos = atomicAdd(cursor + s, 1);
  if (a < 0 || pos >= len || (long long)a + pos >= max_open) return;
  const int wt = w[(size_t)t * (size_t)n_rows + (size_t)r];
  rows[a + pos] = make_int2((int)r, wt | (y[r] ? 256 : 0));
}

// One block per open slot; dynamic LDS = 40 B per feature (the HrfTables
// entries). Wavefront v takes features v, v + 4, ...: per feature it zeroes
// its private 2-plane i32 histogram (2 KB of LDS), adds the slot's rows to it
// and runs hrf_scan_feature over it; hrf_pick_split ends the block. The rows
// pass through LDS in pieces of HRF_SEG_CHUNK, so a slot of any length works;
// a slot that fits one piece (nearly all of a deep level) is staged once, a
// longer one is staged again for every round of 4 features. bins_rm is the
// row-major u8[N, F] copy of the bins: the 4 wavefronts read neighbouring
// bytes of the same row, and later rounds find the row's line in cache. An
// i32 bin sum is at most rows * 255 < 2^31: the wrapper refuses N * 255 >=
// 2^31.
__global__ __launch_bounds__(HGBT_BLOCK) void hrf_seg_split_kernel(
    const int2* __restrict__ rows, const int* __restrict__ seg_off,
    const uint8_t* __restrict__ bins_rm, const int* __restrict__ bin_off,
    const int* __restrict__ slot_meta, long long n_rows, int n_feat,
    int max_open, int max_features, long long min_leaf,
    unsigned long long seed, long long* __restrict__ out)
{
  extern __shared__ long long hrf_seg_lds[];
  __shared__ int2 stage[HRF_SEG_CHUNK];
  __shared__ int wave_hist[HGBT_BLOCK / 64][2 * HGBT_MAX_BINS];
  __shared__ long long tot[2];
  __shared__ int r_star;
  __shared__ HrfPick wave_pick[HGBT_BLOCK / 64];
  const int k = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  if (n_feat > HRF_MAX_FEATS) return;  // the wrapper refuses this too
  const int a = seg_off[k];
  const int len = seg_off[k + 1] - a;
  if (a < 0 || len < 0 || (long long)a + len > max_open) return;
  int* f_bin = reinterpret_cast<int*>(hrf_seg_lds + 4 * n_feat);
  const HrfTables t = {
      reinterpret_cast<double*>(hrf_seg_lds),
      reinterpret_cast<unsigned long long*>(hrf_seg_lds + n_feat),
      hrf_seg_lds + 2 * n_feat, hrf_seg_lds + 3 * n_feat,
      f_bin, f_bin + n_feat, tot, &r_star, wave_pick};

  if (tid == 0) { r_star = n_feat; tot[0] = tot[1] = 0; }
  const int n_chunks = (len + HRF_SEG_CHUNK - 1) / HRF_SEG_CHUNK;
  int* hp = wave_hist[wave];
  int* hw = hp + HGBT_MAX_BINS;
  for (int f0 = 0; f0 < n_feat; f0 += HGBT_BLOCK / 64) {
    const int f = f0 + wave;
    int nb = 0;
    if (f < n_feat) {
      nb = bin_off[f + 1] - bin_off[f];  // only the width is used here
      if (nb <= 0 || nb > HGBT_MAX_BINS) nb = 0;
    }
    for (int i = lane; i < 2 * HGBT_MAX_BINS; i += 64) hp[i] = 0;
    for (int c = 0; c < n_chunks; ++c) {
      const int c0 = c * HRF_SEG_CHUNK;
      const int cn = min(HRF_SEG_CHUNK, len - c0);
      if (n_chunks > 1 || f0 == 0) {
        __syncthreads();  // the piece staged before has been read
        for (int i = tid; i < cn; i += HGBT_BLOCK) stage[i] = rows[a + c0 + i];
      }
      __syncthreads();
      if (nb > 0) {
        for (int i = lane; i < cn; i += 64) {
          const int2 e = stage[i];
          if (e.x < 0 || e.x >= n_rows) continue;
          const int b = bins_rm[(size_t)e.x * (size_t)n_feat + (size_t)f];
          if (b >= nb) continue;
          const int wt = e.y & 255;
          if (e.y & 256) atomicAdd(hp + b, wt);
          atomicAdd(hw + b, wt);
        }
      }
    }
    __syncthreads();  // the wavefront's histogram is complete and visible
    if (f < n_feat) hrf_scan_feature(hp, hw, nb, f, lane, min_leaf, t);
  }
  hrf_pick_split(t, n_feat, max_features, seed, slot_meta[2 * k], slot_meta[2 * k + 1],
                 out + (size_t)k * HRF_REC);
}

// Shared argument checks of the three hrf wrappers: returns TB.
int64_t hrf_check_batch(const torch::Tensor& bins, const torch::Tensor& node,
                        const torch::Tensor& slot_off, int64_t n_slots) {
  TORCH_CHECK(bins.is_cuda() && bins.scalar_type() == torch::kUInt8 &&
              bins.dim() == 2 && bins.is_contiguous(),
              "bins must be a contiguous u8[F, N] GPU tensor");
  hgbt_check(node, bins, torch::kInt32, "node");
  hgbt_check(slot_off, bins, torch::kInt32, "slot_off");
  TORCH_CHECK(node.dim() == 2 && node.size(1) == bins.size(1), "node must be i32[TB, N]");
  const int64_t TB = node.size(0);
  TORCH_CHECK(TB >= 1 && TB <= 65535, "tree batch out of range (1..65535)");
  TORCH_CHECK(slot_off.dim() == 1 && slot_off.size(0) == TB + 1,
              "slot_off must be i32[TB+1]");
  TORCH_CHECK(n_slots >= 0, "n_slots must be >= 0");
  return TB;
}

// Level histogram i64[n_slots, 2, total_bins] of a tree batch. lds_entries is
// the int32 entry count of the largest (tree, feature group) slab, or 0 to
// take the direct-global path. n_slots must equal slot_off[TB].
torch::Tensor hrf_hist(
    torch::Tensor bins, torch::Tensor bin_off, torch::Tensor grp_off,
    torch::Tensor y, torch::Tensor w, torch::Tensor node, torch::Tensor slot_off,
    int64_t n_slots, int64_t total_bins, int64_t lds_entries,
    int64_t rows_per_block)
{
  const int64_t TB = hrf_check_batch(bins, node, slot_off, n_slots);
  const int64_t F = bins.size(0), N = bins.size(1);
  hgbt_check(bin_off, bins, torch::kInt32, "bin_off");
  hgbt_check(grp_off, bins, torch::kInt32, "grp_off");
  hgbt_check(y, bins, torch::kUInt8, "y");
  hgbt_check(w, bins, torch::kUInt8, "w");
  TORCH_CHECK(F >= 1 && F <= HRF_MAX_FEATS, "feature count out of range (1..",
              HRF_MAX_FEATS, ")");
  TORCH_CHECK(bin_off.dim() == 1 && bin_off.size(0) == F + 1, "bin_off must be i32[F+1]");
  TORCH_CHECK(grp_off.dim() == 1 && grp_off.size(0) >= 2 && grp_off.size(0) <= F + 1,
              "grp_off must be i32[groups+1]");
  TORCH_CHECK(y.numel() == N, "y must have one entry per row");
  TORCH_CHECK(w.dim() == 2 && w.size(0) == TB && w.size(1) == N, "w must be u8[TB, N]");
  TORCH_CHECK(total_bins >= 1 && total_bins <= F * HGBT_MAX_BINS &&
              n_slots * 2 * total_bins < (int64_t(1) << 31),
              "histogram shape out of range");
  TORCH_CHECK(rows_per_block >= 1 && rows_per_block <= HRF_MAX_ROWS_PER_BLOCK,
              "rows_per_block must be in [1, ", HRF_MAX_ROWS_PER_BLOCK, "]");
  TORCH_CHECK(lds_entries >= 0 &&
              (size_t)lds_entries * sizeof(int) <= HGBT_LDS_BYTES_MAX,
              "LDS slab larger than the CU's LDS");

  c10::hip::HIPGuard guard((c10::DeviceIndex)bins.get_device());
  auto hist = torch::zeros({n_slots, 2, total_bins},
      torch::TensorOptions().dtype(torch::kInt64).device(bins.device()));
  if (N == 0 || n_slots == 0) return hist;
  const int64_t row_blocks = (N + rows_per_block - 1) / rows_per_block;
  TORCH_CHECK(row_blocks < (int64_t(1) << 31), "too many rows");

  static bool lds_opt_in = false;
  if (!lds_opt_in) {  // dynamic LDS above 64 KiB needs the opt-in once
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&hrf_hist_kernel),
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)HGBT_LDS_BYTES_MAX));
    lds_opt_in = true;
  }
  hipStream_t stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(hrf_hist_kernel,
      dim3((unsigned)row_blocks, (unsigned)(grp_off.size(0) - 1), (unsigned)TB),
      dim3(HGBT_BLOCK), (size_t)lds_entries * sizeof(int), stream,
      bins.data_ptr<uint8_t>(), bin_off.data_ptr<int>(), grp_off.data_ptr<int>(),
      y.data_ptr<uint8_t>(), w.data_ptr<uint8_t>(), node.data_ptr<int>(),
      slot_off.data_ptr<int>(),
      (long long)N, (int)F, (int)n_slots, (int)total_bins, (int)rows_per_block,
      (int)lds_entries,
      reinterpret_cast<unsigned long long*>(hist.data_ptr<int64_t>()));
  HIP_CHECK(hipGetLastError());
  return hist;
}

// Chosen split per open slot: i64[n_slots, HRF_REC] records. seed is the
// 64-bit key seed, passed as its two's-complement int64.
torch::Tensor hrf_split(torch::Tensor hist, torch::Tensor bin_off,
                        torch::Tensor slot_meta, int64_t max_features,
                        int64_t min_leaf, int64_t seed)
{
  TORCH_CHECK(hist.is_cuda() && hist.scalar_type() == torch::kInt64 &&
              hist.dim() == 3 && hist.size(1) == 2 && hist.is_contiguous(),
              "hist must be a contiguous i64[n_slots, 2, total_bins] GPU tensor");
  hgbt_check(bin_off, hist, torch::kInt32, "bin_off");
  hgbt_check(slot_meta, hist, torch::kInt32, "slot_meta");
  const int64_t K = hist.size(0), F = bin_off.numel() - 1;
  TORCH_CHECK(bin_off.dim() == 1 && F >= 1 && F <= HRF_MAX_FEATS,
              "bin_off must be i32[F+1] with F in 1..", HRF_MAX_FEATS);
  TORCH_CHECK(slot_meta.dim() == 2 && slot_meta.size(0) == K && slot_meta.size(1) == 2,
              "slot_meta must be i32[n_slots, 2]");
  TORCH_CHECK(max_features >= 1 && max_features <= F, "max_features must be in [1, F]");
  TORCH_CHECK(min_leaf >= 1, "min_leaf must be >= 1");
  c10::hip::HIPGuard guard((c10::DeviceIndex)hist.get_device());
  auto out = torch::zeros({K, HRF_REC},
      torch::TensorOptions().dtype(torch::kInt64).device(hist.device()));
  if (K == 0) return out;
  hipStream_t stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(hrf_split_kernel, dim3((unsigned)K), dim3(HGBT_BLOCK), 0, stream,
      reinterpret_cast<const long long*>(hist.data_ptr<int64_t>()),
      bin_off.data_ptr<int>(), slot_meta.data_ptr<int>(), (int)F, (int)hist.size(2),
      (int)max_features, (long long)min_leaf, (unsigned long long)seed,
      reinterpret_cast<long long*>(out.data_ptr<int64_t>()));
  HIP_CHECK(hipGetLastError());
  return out;
}

// Move every open row of every tree to its child (in place on `node`).
void hrf_route(torch::Tensor bins, torch::Tensor table, torch::Tensor node,
               torch::Tensor slot_off)
{
  TORCH_CHECK(table.dim() == 2 && table.size(1) == 4, "table must be i32[n_slots, 4]");
  const int64_t K = table.size(0);
  const int64_t TB = hrf_check_batch(bins, node, slot_off, K);
  hgbt_check(table, bins, torch::kInt32, "table");
  const int64_t N = bins.size(1);
  if (N == 0 || K == 0) return;
  const int64_t blocks = (N + HGBT_BLOCK - 1) / HGBT_BLOCK;
  TORCH_CHECK(blocks < (int64_t(1) << 31), "too many rows");
  c10::hip::HIPGuard guard((c10::DeviceIndex)bins.get_device());
  hipStream_t stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(hrf_route_kernel, dim3((unsigned)blocks, (unsigned)TB),
      dim3(HGBT_BLOCK), 0, stream,
      bins.data_ptr<uint8_t>(), reinterpret_cast<const int4*>(table.data_ptr<int>()),
      slot_off.data_ptr<int>(), (long long)N, (int)bins.size(0), (int)K,
      node.data_ptr<int>());
  HIP_CHECK(hipGetLastError());
}

// Bucket the open rows of a level by slot: {seg_off i32[n_slots+1], rows
// i32[max_open, 2]}; slot s owns rows[seg_off[s] : seg_off[s+1]], entries
// {row id, w | y << 8}. max_open bounds the open rows from above (the host
// passes the open slots' weight, and a row weighs at least 1); entries past
// seg_off[n_slots] stay unwritten. n_slots must equal slot_off[TB].
std::vector<torch::Tensor> hrf_seg_build(
    torch::Tensor bins, torch::Tensor y, torch::Tensor w, torch::Tensor node,
    torch::Tensor slot_off, int64_t n_slots, int64_t max_open)
{
  const int64_t TB = hrf_check_batch(bins, node, slot_off, n_slots);
  const int64_t N = bins.size(1);
  hgbt_check(y, bins, torch::kUInt8, "y");
  hgbt_check(w, bins, torch::kUInt8, "w");
  TORCH_CHECK(y.numel() == N, "y must have one entry per row");
  TORCH_CHECK(w.dim() == 2 && w.size(0) == TB && w.size(1) == N, "w must be u8[TB, N]");
  TORCH_CHECK(N * 255 < (int64_t(1) << 31),
              "too many rows for the int32 sums of the segmented level");
  TORCH_CHECK(n_slots < (int64_t(1) << 31) - 1, "too many slots");
  TORCH_CHECK(max_open >= 0 && max_open < (int64_t(1) << 31), "max_open out of range");

  c10::hip::HIPGuard guard((c10::DeviceIndex)bins.get_device());
  const auto i32 = torch::TensorOptions().dtype(torch::kInt32).device(bins.device());
  auto seg_off = torch::zeros({n_slots + 1}, i32);
  auto rows = torch::empty({max_open, 2}, i32);
  if (N == 0 || n_slots == 0) return {seg_off, rows};
  auto work = torch::zeros({2, n_slots}, i32);  // counts, then the cursors
  int* cnt = work.data_ptr<int>();
  int* cursor = cnt + n_slots;
  const int64_t blocks = (N + HGBT_BLOCK - 1) / HGBT_BLOCK;
  const dim3 grid((unsigned)blocks, (unsigned)TB);
  hipStream_t stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(hrf_seg_count_kernel, grid, dim3(HGBT_BLOCK), 0, stream,
      w.data_ptr<uint8_t>(), node.data_ptr<int>(), slot_off.data_ptr<int>(),
      (long long)N, (int)n_slots, cnt);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(hrf_seg_scan_kernel, dim3(1), dim3(HRF_SCAN_BLOCK), 0, stream,
      cnt, (int)n_slots, seg_off.data_ptr<int>());
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(hrf_seg_scatter_kernel, grid, dim3(HGBT_BLOCK), 0, stream,
      w.data_ptr<uint8_t>(), y.data_ptr<uint8_t>(), node.data_ptr<int>(),
      slot_off.data_ptr<int>(), seg_off.data_ptr<int>(), (long long)N, (int)n_slots,
      (int)max_open, cursor, reinterpret_cast<int2*>(rows.data_ptr<int>()));
  HIP_CHECK(hipGetLastError());
  return {seg_off, rows};
}

// Chosen split per open slot from the bucketed rows of hrf_seg_build:
// hrf_split's i64[n_slots, HRF_REC] records without a level histogram.
// bins_rm is the row-major u8[N, F] copy of the bins.
torch::Tensor hrf_seg_split(torch::Tensor rows, torch::Tensor seg_off,
                            torch::Tensor bins_rm, torch::Tensor bin_off,
                            torch::Tensor slot_meta, int64_t max_features,
                            int64_t min_leaf, int64_t seed)
{
  TORCH_CHECK(bins_rm.is_cuda() && bins_rm.scalar_type() == torch::kUInt8 &&
              bins_rm.dim() == 2 && bins_rm.is_contiguous(),
              "bins_rm must be a contiguous u8[N, F] GPU tensor");
  hgbt_check(rows, bins_rm, torch::kInt32, "rows");
  hgbt_check(seg_off, bins_rm, torch::kInt32, "seg_off");
  hgbt_check(bin_off, bins_rm, torch::kInt32, "bin_off");
  hgbt_check(slot_meta, bins_rm, torch::kInt32, "slot_meta");
  const int64_t N = bins_rm.size(0), F = bins_rm.size(1);
  const int64_t K = seg_off.numel() - 1;
  TORCH_CHECK(F >= 1 && F <= HRF_MAX_FEATS, "feature count out of range (1..",
              HRF_MAX_FEATS, ")");
  TORCH_CHECK(N * 255 < (int64_t(1) << 31),
              "too many rows for the int32 sums of the segmented level");
  TORCH_CHECK(rows.dim() == 2 && rows.size(1) == 2, "rows must be i32[max_open, 2]");
  TORCH_CHECK(seg_off.dim() == 1 && K >= 0, "seg_off must be i32[n_slots+1]");
  TORCH_CHECK(bin_off.dim() == 1 && bin_off.size(0) == F + 1, "bin_off must be i32[F+1]");
  TORCH_CHECK(slot_meta.dim() == 2 && slot_meta.size(0) == K && slot_meta.size(1) == 2,
              "slot_meta must be i32[n_slots, 2]");
  TORCH_CHECK(max_features >= 1 && max_features <= F, "max_features must be in [1, F]");
  TORCH_CHECK(min_leaf >= 1, "min_leaf must be >= 1");
  c10::hip::HIPGuard guard((c10::DeviceIndex)bins_rm.get_device());
  auto out = torch::zeros({K, HRF_REC},
      torch::TensorOptions().dtype(torch::kInt64).device(bins_rm.device()));
  if (K == 0) return out;
  hipStream_t stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(hrf_seg_split_kernel, dim3((unsigned)K), dim3(HGBT_BLOCK),
      (size_t)F * 40, stream,
      reinterpret_cast<const int2*>(rows.data_ptr<int>()), seg_off.data_ptr<int>(),
      bins_rm.data_ptr<uint8_t>(), bin_off.data_ptr<int>(), slot_meta.data_ptr<int>(),
      (long long)N, (int)F, (int)rows.size(0),
      (int)max_features, (long long)min_leaf, (unsigned long long)seed,
      reinterpret_cast<long long*>(out.data_ptr<int64_t>()));
  HIP_CHECK(hipGetLastError());
  return out;
}

torch::Tensor forest_ilp_bench(
    torch::Tensor codes, torch::Tensor nums,
    torch::Tensor nodes, torch::Tensor off,
    torch::Tensor feat_col, torch::Tensor feat_code,
    torch::Tensor medians, int64_t use_ilp)
{
  check_inputs(codes, nums);
  const int B = (int)codes.size(0);
  const int T = (int)off.size(0) - 1;
  auto acc = torch::zeros({B},
      torch::TensorOptions().dtype(torch::kFloat64).device(codes.device()));
  hipStream_t stream = c10::hip::getCurrentHIPStream();
  const int row_blocks = ceil_div(B, BLOCK);
  int chunks = std::max(1, std::min(ceil_div(2048, row_blocks), T));
  if (use_ilp) {
    const int ilp = (use_ilp == 2 || use_ilp == 4) ? 4 : 2;
    const bool swap = use_ilp >= 3;
    chunks = std::max(1, std::min(ceil_div(2048, row_blocks), (T + ilp - 1) / ilp));
    dim3 grid = swap ? dim3(chunks, row_blocks) : dim3(row_blocks, chunks);
    auto args = std::make_tuple(
        codes.data_ptr<short>(), nums.data_ptr<float>(), medians.data_ptr<float>(),
        reinterpret_cast<const int4*>(nodes.data_ptr<int>()), off.data_ptr<int>(), T,
        feat_col.data_ptr<int>(), feat_code.data_ptr<int>(), B, acc.data_ptr<double>());
    auto launch = [&](auto kernel) {
      std::apply([&](auto... a) {
        hipLaunchKernelGGL(kernel, grid, dim3(BLOCK), 0, stream, a...);
      }, args);
    };
    if (use_ilp == 1) launch(forest_kernel_ilpN<false, 2, false>);
    else if (use_ilp == 2) launch(forest_kernel_ilpN<false, 4, false>);
    else if (use_ilp == 3) launch(forest_kernel_ilpN<false, 2, true>);
    else launch(forest_kernel_ilpN<false, 4, true>);
  } else {
    hipLaunchKernelGGL((forest_kernel<false>), dim3(row_blocks, chunks),
        dim3(BLOCK), 0, stream,
        codes.data_ptr<short>(), nums.data_ptr<float>(), medians.data_ptr<float>(),
        reinterpret_cast<const int4*>(nodes.data_ptr<int>()), off.data_ptr<int>(), T,
        feat_col.data_ptr<int>(), feat_code.data_ptr<int>(), B, acc.data_ptr<double>());
  }
  HIP_CHECK(hipGetLastError());
  return acc;
}

std::vector<torch::Tensor> drift_stats(
    torch::Tensor codes, torch::Tensor nums, torch::Tensor medians,
    torch::Tensor ref_sorted, torch::Tensor rs_off, torch::Tensor cat_off,
    int64_t total_bins)
{
  check_inputs(codes, nums);
  const int B = (int)codes.size(0);
  TORCH_CHECK(B <= MAX_DRIFT_ROWS,
      "drift batch too large for the K-S LDS sort (cap it host-side): ", B);

  auto hist = torch::zeros({total_bins},
      torch::TensorOptions().dtype(torch::kInt32).device(codes.device()));
  auto ks_d = torch::empty({N_NUM},
      torch::TensorOptions().dtype(torch::kFloat32).device(codes.device()));
  auto rs_off64 = rs_off.to(torch::kInt64);

  hipStream_t stream = c10::hip::getCurrentHIPStream();

  const int hist_blocks = std::min(ceil_div(B, BLOCK), 1024);
  hipLaunchKernelGGL(cat_hist_kernel, dim3(hist_blocks), dim3(BLOCK),
      (size_t)total_bins * sizeof(int), stream,
      codes.data_ptr<short>(), B, cat_off.data_ptr<int>(), (int)total_bins,
      hist.data_ptr<int>());

  if (B <= KS_COUNT_MAX_ROWS) {
    const size_t smem = (size_t)std::max(B, BLOCK / 64) * sizeof(float);
    hipLaunchKernelGGL((ks_count_kernel_t<256>), dim3(N_NUM), dim3(BLOCK),
        smem, stream,
        nums.data_ptr<float>(), medians.data_ptr<float>(), N_NUM, B,
        ref_sorted.data_ptr<float>(), rs_off64.data_ptr<int64_t>(),
        ks_d.data_ptr<float>());
  } else {
    int m_pow2 = 1;
    while (m_pow2 < B) m_pow2 <<= 1;
    // LDS must also hold one cross-wave reduction slot per wave
    m_pow2 = std::max(m_pow2, BLOCK / 64);
    hipLaunchKernelGGL((ks_kernel_t<256>), dim3(N_NUM), dim3(BLOCK),
        (size_t)m_pow2 * sizeof(float), stream,
        nums.data_ptr<float>(), medians.data_ptr<float>(), N_NUM, B, m_pow2,
        /*ref_lds=*/0, ref_sorted.data_ptr<float>(),
        rs_off64.data_ptr<int64_t>(), ks_d.data_ptr<float>());
  }
  HIP_CHECK(hipGetLastError());

  return {hist, ks_d};
}

// ---------------------------------------------------------------------------
// Dense wide-tabular family (BASELINE config 5: 10M x 1k synthetic).
// dense_score_kernel: fused impute + logistic linear score + robust-z
// outlier flag, one wavefront per row (64 lanes stride the F features with
// coalesced loads; wave shuffle-reduce for the dot product and max-z).
// Drift for this family reuses ks_kernel with n_cols = F and the per-feature
// sorted reference resident in HBM (the 288 GB sizing: a 10M x 1k f32
// reference is 40 GB per GPU).
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(BLOCK) void dense_score_kernel(
    const float* __restrict__ x,        // [B, F]
    const float* __restrict__ medians,  // [F]
    const float* __restrict__ inv_scale,// [F] 1/(IQR) robust scale
    const float* __restrict__ w,        // [F]
    float bias,
    float z_threshold,
    int n_rows,
    int n_feat,
    double* __restrict__ proba,         // [B]
    double* __restrict__ iscore,        // [B] max robust z
    double* __restrict__ outlier)       // [B]
{
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (BLOCK / 64) + wave;
  if (row >= n_rows) return;
  const float* xr = x + (size_t)row * n_feat;

  float acc = 0.0f;
  float zmax = 0.0f;
  for (int f = lane; f < n_feat; f += 64) {
    float v = xr[f];
    const float med = medians[f];
    if (isnan(v)) v = med;  // fused median imputation
    acc += v * w[f];
    const float z = fabsf(v - med) * inv_scale[f];
    zmax = fmaxf(zmax, z);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    acc += __shfl_down(acc, off, 64);
    zmax = fmaxf(zmax, __shfl_down(zmax, off, 64));
  }
  if (lane == 0) {
    const double logit = (double)acc + (double)bias;
    proba[row] = 1.0 / (1.0 + exp(-logit));
    iscore[row] = (double)zmax;
    outlier[row] = (zmax > z_threshold) ? 1.0 : 0.0;
  }
}

std::vector<torch::Tensor> dense_score(
    torch::Tensor x, torch::Tensor medians, torch::Tensor inv_scale,
    torch::Tensor w, double bias, double z_threshold)
{
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == torch::kFloat32 && x.is_contiguous());
  const int B = (int)x.size(0);
  const int F = (int)x.size(1);
  TORCH_CHECK(medians.numel() == F && w.numel() == F && inv_scale.numel() == F);
  auto opts = torch::TensorOptions().dtype(torch::kFloat64).device(x.device());
  auto proba = torch::empty({B}, opts);
  auto iscore = torch::empty({B}, opts);
  auto outlier = torch::empty({B}, opts);
  hipStream_t stream = c10::hip::getCurrentHIPStream();
  const int rows_per_block = BLOCK / 64;
  hipLaunchKernelGGL(dense_score_kernel,
      dim3(ceil_div(B, rows_per_block)), dim3(BLOCK), 0, stream,
      x.data_ptr<float>(), medians.data_ptr<float>(), inv_scale.data_ptr<float>(),
      w.data_ptr<float>(), (float)bias, (float)z_threshold, B, F,
      proba.data_ptr<double>(), iscore.data_ptr<double>(), outlier.data_ptr<double>());
  HIP_CHECK(hipGetLastError());
  return {proba, iscore, outlier};
}

// Fused impute + transpose for the large-batch dense drift path:
// x [B, F] row-major -> xt [F, B] row-major with NaN -> median, one pass
// through an LDS tile (32x32, +1 padding column against bank conflicts).
__global__ __launch_bounds__(256) void impute_transpose_kernel(
    const float* __restrict__ x,   // [B, F]
    const float* __restrict__ medians,  // [F]
    int n_rows,
    int n_feat,
    float* __restrict__ xt)        // [F, B]
{
  __shared__ float tile[32][33];
  const int f0 = blockIdx.x * 32;
  const int r0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31;   // feature within tile on load
  const int ty = threadIdx.x >> 5;   // row group (8 rows per pass)
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = r0 + ty + k * 8;
    const int f = f0 + tx;
    float v = 0.0f;
    if (r < n_rows && f < n_feat) {
      v = x[(size_t)r * n_feat + f];
      if (isnan(v)) v = medians[f];
    }
    tile[ty + k * 8][tx] = v;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int f = f0 + ty + k * 8;   // feature on store
    const int r = r0 + tx;           // row on store (coalesced)
    if (f < n_feat && r < n_rows) xt[(size_t)f * n_rows + r] = tile[tx][ty + k * 8];
  }
}

torch::Tensor impute_transpose(torch::Tensor x, torch::Tensor medians) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == torch::kFloat32 && x.is_contiguous());
  const int B = (int)x.size(0);
  const int F = (int)x.size(1);
  TORCH_CHECK((int)medians.numel() == F, "median size mismatch");
  auto xt = torch::empty({F, B},
      torch::TensorOptions().dtype(torch::kFloat32).device(x.device()));
  hipStream_t stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(impute_transpose_kernel,
      dim3(ceil_div(F, 32), ceil_div(B, 32)), dim3(256), 0, stream,
      x.data_ptr<float>(), medians.data_ptr<float>(), B, F,
      xt.data_ptr<float>());
  HIP_CHECK(hipGetLastError());
  return xt;
}

// Scan-only K-S for pre-sorted batch columns (large-B dense path: the sort
// goes through rocPRIM (torch.sort), then this kernel fills the chip with
// (feature x row-chunk) blocks; per-feature max via f32-bit atomicMax).
__global__ __launch_bounds__(BLOCK) void ks_scan_kernel(
    const float* __restrict__ xs,         // [F, B] row-contiguous, each row sorted
    int n_cols,
    int n_rows,
    const float* __restrict__ ref_sorted,
    const int64_t* __restrict__ rs_off,
    unsigned int* __restrict__ ks_bits)   // [F] f32 bits, pre-zeroed
{
  const int j = blockIdx.x;
  const int i = blockIdx.y * blockDim.x + threadIdx.x;
  const int m = n_rows;
  const int64_t lo = rs_off[j];
  const int n = (int)(rs_off[j + 1] - lo);
  const float* __restrict__ ref = ref_sorted + lo;
  const float* __restrict__ col = xs + (size_t)j * n_rows;  // contiguous

  double dmax = 0.0;
  if (i < m) {
    const float b = col[i];
    int l = 0, r = n;
    while (l < r) { const int mid = (l + r) >> 1; if (ref[mid] < b) l = mid + 1; else r = mid; }
    const int sl = l;
    r = n;
    while (l < r) { const int mid = (l + r) >> 1; if (ref[mid] <= b) l = mid + 1; else r = mid; }
    const int sr = l;
    int bl = 0; r = i;  // tie-run bounds within the sorted column
    while (bl < r) { const int mid = (bl + r) >> 1;
      if (col[mid] < b) bl = mid + 1; else r = mid; }
    int br = i + 1; r = m;
    while (br < r) { const int mid = (br + r) >> 1;
      if (col[mid] <= b) br = mid + 1; else r = mid; }
    const double fl = fabs((double)sl / n - (double)bl / m);
    const double fr = fabs((double)sr / n - (double)br / m);
    dmax = fmax(fl, fr);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    dmax = fmax(dmax, __shfl_down(dmax, off, 64));
  if ((threadIdx.x & 63) == 0 && dmax > 0.0)
    atomicMax(&ks_bits[j], __float_as_uint((float)dmax));
}

torch::Tensor ks_stats_sorted(
    torch::Tensor xs_sorted, torch::Tensor ref_sorted, torch::Tensor rs_off)
{
  TORCH_CHECK(xs_sorted.is_cuda() && xs_sorted.scalar_type() == torch::kFloat32
              && xs_sorted.is_contiguous());
  const int F = (int)xs_sorted.size(0);  // [F, B]: per-feature sorted rows
  const int B = (int)xs_sorted.size(1);
  TORCH_CHECK((int)rs_off.size(0) == F + 1, "rs_off size mismatch");
  auto bits = torch::zeros({F},
      torch::TensorOptions().dtype(torch::kInt32).device(xs_sorted.device()));
  hipStream_t stream = c10::hip::getCurrentHIPStream();
  auto rs_off64 = rs_off.to(torch::kInt64);
  hipLaunchKernelGGL(ks_scan_kernel, dim3(F, ceil_div(B, BLOCK)), dim3(BLOCK), 0, stream,
      xs_sorted.data_ptr<float>(), F, B,
      ref_sorted.data_ptr<float>(), rs_off64.data_ptr<int64_t>(),
      reinterpret_cast<unsigned int*>(bits.data_ptr<int>()));
  HIP_CHECK(hipGetLastError());
  return bits.view(torch::kFloat32);
}

// Generic exact K-S D over any column count (dense drift path; the credit
// path embeds the same kernel in its session graph).
torch::Tensor ks_stats(
    torch::Tensor nums, torch::Tensor medians,
    torch::Tensor ref_sorted, torch::Tensor rs_off,
    int64_t block, int64_t ref_lds)
{
  TORCH_CHECK(nums.is_cuda() && nums.scalar_type() == torch::kFloat32 && nums.is_contiguous());
  const int B = (int)nums.size(0);
  const int F = (int)nums.size(1);
  TORCH_CHECK(B <= MAX_DRIFT_ROWS, "K-S batch too large: ", B);
  TORCH_CHECK((int)rs_off.size(0) == F + 1, "rs_off size mismatch");
  TORCH_CHECK(block == 256 || block == 512, "block must be 256 or 512");
  auto ks_d = torch::empty({F},
      torch::TensorOptions().dtype(torch::kFloat32).device(nums.device()));
  hipStream_t stream = c10::hip::getCurrentHIPStream();
  int m_pow2 = (int)block / 64;  // >= one reduction slot per wave
  while (m_pow2 < B) m_pow2 <<= 1;
  size_t smem = (size_t)m_pow2 * sizeof(float);
  auto rs_off64 = rs_off.to(torch::kInt64);
  if (ref_lds) {
    int64_t maxr = 0;
    auto ro = rs_off64.cpu();
    auto* rp = ro.data_ptr<int64_t>();
    for (int j = 0; j < F; ++j) maxr = std::max<int64_t>(maxr, rp[j + 1] - rp[j]);
    smem += (size_t)maxr * sizeof(float);
    TORCH_CHECK(smem <= KS_LDS_BYTES_MAX, "ref too large for LDS");
  }
  if (block == 512)
    hipLaunchKernelGGL((ks_kernel_t<512>), dim3(F), dim3(512), smem, stream,
        nums.data_ptr<float>(), medians.data_ptr<float>(), F, B, m_pow2,
        (int)ref_lds, ref_sorted.data_ptr<float>(),
        rs_off64.data_ptr<int64_t>(), ks_d.data_ptr<float>());
  else
    hipLaunchKernelGGL((ks_kernel_t<256>), dim3(F), dim3(256), smem, stream,
        nums.data_ptr<float>(), medians.data_ptr<float>(), F, B, m_pow2,
        (int)ref_lds, ref_sorted.data_ptr<float>(),
        rs_off64.data_ptr<int64_t>(), ks_d.data_ptr<float>());
  HIP_CHECK(hipGetLastError());
  return ks_d;
}

// ---------------------------------------------------------------------------
// MMD permutation test (creditcore/mmd.py): W = K . ind without ever holding
// the RBF Gram matrix K (4 GiB in f32 at 32,768 pooled rows). Both products
// run on the matrix cores in f32 (v_mfma_f32_16x16x4_f32):
//
//   GEMM 1   S[j, i] = z_j . z_i            (transposed on purpose, see below)
//   epilogue k[j, i] = exp(-gamma max(n_i + n_j - 2 S, 0)), 0 on the diagonal
//   GEMM 2   Wt[q, i] += sum_j ind[j, q] k[j, i]
//
// A 256-thread block owns 64 rows i (16 per wave) and the columns
// j in [y * cols_per_block, ...), walked in tiles of 64. Per tile the z rows
// of both sides stream through LDS in 64-wide d-chunks (so D is not bounded
// by registers) and the tile's indicator bytes sit in LDS, q-major, one dword
// per four consecutive j.
//
// Operand layouts of the 16x16x4 f32 MFMA (lane l, h = l % 16, g = l / 16):
// A holds A[h][k = g], B holds B[k = g][h], the accumulator register r holds
// D[4 g + r][h]. With S computed as rows j x columns i a lane's four
// accumulators are k[j = 4 g + r][i = h]; j is the summation index of GEMM 2
// and its order inside the tile is free, so register r is fed unchanged as
// the B operand of step r (summation slot g stands for j = 4 g + r) and the
// A operand is ind[4 g + r][q = h]: byte r of the one dword the lane reads.
// K never takes a trip through LDS to change layout. The same freedom is used
// on d in GEMM 1: a lane reads d = 16 kk + 4 g .. + 3 of its row as one
// float4 for four steps, on both operands alike.
//
// Every block writes its own f32 slab part[y][i][0 .. Qp): no atomics, no
// pre-zeroed output; mmd_sum_kernel adds the slabs in f64 in split order, so
// the result is bit-identical run to run.
// ---------------------------------------------------------------------------

#define MMD_BLOCK 256
#define MMD_TILE 64       // rows i of a block; rows j of one step
#define MMD_DC 64         // d-chunk staged in LDS
#define MMD_ZLD 68        // LDS row stride of a z tile (floats): float4 reads
                          // of 16 rows land on 16 distinct 4-bank groups
#define MMD_ILD 17        // LDS row stride of the indicator tile (dwords)
#define MMD_QT_MAX 16     // 16-wide q tiles: Qp <= 256
#define MMD_MAX_POOLED 32768
#define MMD_MAX_DP 4096

// The MMD kernels are generated without packed f32 VALU instructions
// (v_pk_fma_f32 and kin); per function, so that every other kernel of this
// file keeps its code generation.
#if defined(__HIP_DEVICE_COMPILE__)
#define MMD_NO_PACKED_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define MMD_NO_PACKED_F32
#endif

typedef float mmd_f4 __attribute__((ext_vector_type(4)));

MMD_NO_PACKED_F32 __global__ __launch_bounds__(MMD_BLOCK) void mmd_perm_kernel(
    const float* __restrict__ z,        // [N, Dp]
    const float* __restrict__ norms,    // [Np], 0 past N
    const uint8_t* __restrict__ ind_t,  // [Qp, Np], 0 past Q and past N
    float* __restrict__ part,           // [splits, rows, Qp]
    int N, int Np, int Dp, int nqt, int cols_per_block, int row0, int rows,
    float gamma)
{
  __shared__ __attribute__((aligned(16))) float zi_s[MMD_TILE * MMD_ZLD];
  __shared__ __attribute__((aligned(16))) float zj_s[MMD_TILE * MMD_ZLD];
  __shared__ unsigned ind_s[MMD_QT_MAX * 16 * MMD_ILD];

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int h = lane & 15, g = lane >> 4;
  const int i_base = row0 + (int)blockIdx.x * MMD_TILE;
  const int my_i = i_base + wave * 16 + h;
  const int j_begin = (int)blockIdx.y * cols_per_block;
  const int j_end = min(j_begin + cols_per_block, N);
  const int Qp = nqt * 16;
  const float n_i = norms[min(my_i, Np - 1)];
  const bool i_ok = my_i < N;
  // loader roles: a float4 column and four rows of each z tile per thread
  const int ld_c = tid & 15, ld_r = tid >> 4;
  // one d-chunk: the block's own rows are staged once, not once per j tile
  const bool zi_once = Dp <= MMD_DC;

  mmd_f4 acc[MMD_QT_MAX];
#pragma unroll
  for (int qt = 0; qt < MMD_QT_MAX; ++qt) acc[qt] = mmd_f4{0.f, 0.f, 0.f, 0.f};

  for (int j0 = j_begin; j0 < j_end; j0 += MMD_TILE) {
    mmd_f4 s[4];
#pragma unroll
    for (int js = 0; js < 4; ++js) s[js] = mmd_f4{0.f, 0.f, 0.f, 0.f};

    for (int d0 = 0; d0 < Dp; d0 += MMD_DC) {
      __syncthreads();  // the previous chunk (and tile) is consumed
      const int d = d0 + 4 * ld_c;  // Dp % 4 == 0: d < Dp covers d + 3
      const bool load_i = !zi_once || j0 == j_begin;  // uniform
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int row = ld_r + 16 * k;
        const int gi = i_base + row, gj = j0 + row;
        mmd_f4 vi = mmd_f4{0.f, 0.f, 0.f, 0.f}, vj = vi;
        if (load_i && d < Dp && gi < N)
          vi = *reinterpret_cast<const mmd_f4*>(z + (size_t)gi * Dp + d);
        if (d < Dp && gj < N)
          vj = *reinterpret_cast<const mmd_f4*>(z + (size_t)gj * Dp + d);
        if (load_i)
          *reinterpret_cast<mmd_f4*>(&zi_s[row * MMD_ZLD + 4 * ld_c]) = vi;
        *reinterpret_cast<mmd_f4*>(&zj_s[row * MMD_ZLD + 4 * ld_c]) = vj;
      }
      if (d0 == 0) {
        // indicator tile, q-major: 16 dwords (64 j) per q; j0 + 63 < Np
        for (int q = ld_r; q < Qp; q += 16)
          ind_s[q * MMD_ILD + ld_c] = *reinterpret_cast<const unsigned*>(
              ind_t + (size_t)q * Np + j0 + 4 * ld_c);
      }
      __syncthreads();

#pragma unroll
      for (int kk = 0; kk < MMD_DC / 16; ++kk) {
        if (d0 + kk * 16 >= Dp) continue;  // uniform
        const mmd_f4 b = *reinterpret_cast<const mmd_f4*>(
            &zi_s[(wave * 16 + h) * MMD_ZLD + kk * 16 + 4 * g]);
#pragma unroll
        for (int js = 0; js < 4; ++js) {
          const mmd_f4 a = *reinterpret_cast<const mmd_f4*>(
              &zj_s[(js * 16 + h) * MMD_ZLD + kk * 16 + 4 * g]);
          s[js] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, s[js], 0, 0, 0);
          s[js] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, s[js], 0, 0, 0);
          s[js] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, s[js], 0, 0, 0);
          s[js] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, s[js], 0, 0, 0);
        }
      }
    }

    // epilogue on the accumulators, then GEMM 2 straight from them
#pragma unroll
    for (int js = 0; js < 4; ++js) {
      const int jr = j0 + js * 16 + 4 * g;  // register r is row jr + r
      const mmd_f4 n_j = *reinterpret_cast<const mmd_f4*>(norms + jr);
      mmd_f4 kv;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float d2 = fmaxf(n_i + n_j[r] - 2.0f * s[js][r], 0.0f);
        const float k = expf(-gamma * d2);
        kv[r] = (i_ok && jr + r < N && jr + r != my_i) ? k : 0.0f;
      }
#pragma unroll
      for (int qt = 0; qt < MMD_QT_MAX; ++qt) {
        if (qt >= nqt) continue;  // uniform; keeps acc[] in registers
        const unsigned u = ind_s[(qt * 16 + h) * MMD_ILD + js * 4 + g];
        acc[qt] = __builtin_amdgcn_mfma_f32_16x16x4f32(
            (float)(u & 0xffu), kv[0], acc[qt], 0, 0, 0);
        acc[qt] = __builtin_amdgcn_mfma_f32_16x16x4f32(
            (float)((u >> 8) & 0xffu), kv[1], acc[qt], 0, 0, 0);
        acc[qt] = __builtin_amdgcn_mfma_f32_16x16x4f32(
            (float)((u >> 16) & 0xffu), kv[2], acc[qt], 0, 0, 0);
        acc[qt] = __builtin_amdgcn_mfma_f32_16x16x4f32(
            (float)(u >> 24), kv[3], acc[qt], 0, 0, 0);
      }
    }
  }

  // acc[qt][r] is Wt[q = 16 qt + 4 g + r][i = my_i]: one float4 per q tile
  if (i_ok && my_i < row0 + rows) {
    float* out = part + ((size_t)blockIdx.y * rows + (my_i - row0)) * Qp + 4 * g;
#pragma unroll
    for (int qt = 0; qt < MMD_QT_MAX; ++qt) {
      if (qt >= nqt) continue;
      *reinterpret_cast<mmd_f4*>(out + qt * 16) = acc[qt];
    }
  }
}

// W[i, q] = sum over splits of part[s, i, q], added in f64 in split order.
MMD_NO_PACKED_F32 __global__ __launch_bounds__(BLOCK) void mmd_sum_kernel(
    const float* __restrict__ part, double* __restrict__ w,
    int splits, long long rows, int Q, int Qp)
{
  const long long e = (long long)blockIdx.x * BLOCK + threadIdx.x;
  if (e >= rows * Q) return;
  const long long i = e / Q;
  const int q = (int)(e - i * Q);
  double sum = 0.0;
  for (int s = 0; s < splits; ++s)
    sum += (double)part[((size_t)s * rows + i) * Qp + q];
  w[e] = sum;
}

// W[row_begin .. row_begin + row_count) of K . ind as f64[row_count, Q].
// z f32[N, Dp] (D zero-padded to a multiple of 4), norms f32[N] the squared
// row norms, ind u8[N, Q] of 0/1. row_count < 0 takes every row from
// row_begin on; a slice lets the caller split a long launch over the i tiles.
torch::Tensor mmd_perm_w(torch::Tensor z, torch::Tensor norms, double gamma,
                         torch::Tensor ind, int64_t cols_per_block,
                         int64_t row_begin, int64_t row_count)
{
  TORCH_CHECK(z.is_cuda() && z.scalar_type() == torch::kFloat32 &&
              z.dim() == 2 && z.is_contiguous(),
              "z must be a contiguous f32[N, Dp] GPU tensor");
  const int64_t N = z.size(0), Dp = z.size(1);
  TORCH_CHECK(N >= 2 && N <= MMD_MAX_POOLED, "pooled rows out of range: ", N);
  TORCH_CHECK(Dp >= 4 && Dp % 4 == 0 && Dp <= MMD_MAX_DP,
              "Dp must be a multiple of 4 in [4, ", MMD_MAX_DP, "]");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(z.data_ptr<float>()) % 16 == 0,
              "z must be 16-byte aligned (rows are read as float4)");
  TORCH_CHECK(norms.is_cuda() && norms.device() == z.device() &&
              norms.scalar_type() == torch::kFloat32 && norms.dim() == 1 &&
              norms.size(0) == N && norms.is_contiguous(),
              "norms must be a contiguous f32[N] tensor on z's GPU");
  TORCH_CHECK(ind.is_cuda() && ind.device() == z.device() &&
              ind.scalar_type() == torch::kUInt8 && ind.dim() == 2 &&
              ind.size(0) == N && ind.is_contiguous(),
              "ind must be a contiguous u8[N, Q] tensor on z's GPU");
  const int64_t Q = ind.size(1);
  TORCH_CHECK(Q >= 1 && Q <= MMD_QT_MAX * 16,
              "Q = P + 2 must be at most ", MMD_QT_MAX * 16, " (P <= 254)");
  TORCH_CHECK(cols_per_block >= MMD_TILE && cols_per_block % MMD_TILE == 0,
              "cols_per_block must be a positive multiple of ", MMD_TILE);
  TORCH_CHECK(std::isfinite(gamma) && gamma > 0.0, "gamma must be positive");
  if (row_count < 0) row_count = N - row_begin;
  TORCH_CHECK(row_begin >= 0 && row_begin % MMD_TILE == 0 && row_count >= 1 &&
              row_begin + row_count <= N,
              "row slice must start on a tile and lie inside [0, N)");

  c10::hip::HIPGuard guard((c10::DeviceIndex)z.get_device());
  const int64_t Np = (N + MMD_TILE - 1) / MMD_TILE * MMD_TILE;
  const int64_t nqt = (Q + 15) / 16, Qp = nqt * 16;
  const int64_t splits = (N + cols_per_block - 1) / cols_per_block;
  // padded operands: the kernel reads whole tiles of these two unchecked
  auto norms_p = torch::zeros({Np}, norms.options());
  norms_p.slice(0, 0, N).copy_(norms);
  auto ind_t = torch::zeros({Qp, Np}, ind.options());
  ind_t.slice(0, 0, Q).slice(1, 0, N).copy_(ind.t());
  auto part = torch::empty({splits, row_count, Qp}, z.options());
  auto w = torch::empty({row_count, Q}, z.options().dtype(torch::kFloat64));

  hipStream_t stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(mmd_perm_kernel,
      dim3((unsigned)((row_count + MMD_TILE - 1) / MMD_TILE), (unsigned)splits),
      dim3(MMD_BLOCK), 0, stream,
      z.data_ptr<float>(), norms_p.data_ptr<float>(), ind_t.data_ptr<uint8_t>(),
      part.data_ptr<float>(), (int)N, (int)Np, (int)Dp, (int)nqt,
      (int)cols_per_block, (int)row_begin, (int)row_count, (float)gamma);
  HIP_CHECK(hipGetLastError());
  const int64_t total = row_count * Q;
  hipLaunchKernelGGL(mmd_sum_kernel, dim3((unsigned)((total + BLOCK - 1) / BLOCK)),
      dim3(BLOCK), 0, stream, part.data_ptr<float>(), w.data_ptr<double>(),
      (int)splits, (long long)row_count, (int)Q, (int)Qp);
  HIP_CHECK(hipGetLastError());
  return w;
}

// ---------------------------------------------------------------------------
// Nearest-neighbour outlier scores (creditcore/knn.py): the k smallest
// squared distances from every batch row to the rows of a reference sample,
// without ever holding the B x M distance matrix (1 GiB in f32 at the caps).
//
//   GEMM      S[j, i] = zr_j . zb_i   (f32 matrix cores, transposed as in
//                                      mmd_perm_kernel, same LDS d-chunks)
//   epilogue  d2 = max(n_i + n_j - 2 S, 0); key = bits(d2) << 32 | j
//   select    per batch row i the k smallest keys of the block's columns
//
// A 256-thread block owns 64 batch rows i (16 per wave) and the reference
// columns j in [y * cols_per_block, ...), walked in tiles of 64. Because the
// distance tile is computed transposed, accumulator register r of MFMA js is
// d2[j = j0 + 16 js + 4 g + r][i = h]: all 16 accumulators of a lane belong
// to ONE batch row, and the four lanes h, h + 16, h + 32, h + 48 hold that
// row's 64 columns of the tile. A wave therefore selects for its own 16 rows
// with no help from the other waves, and the selection needs no block
// barrier.
//
// Selection state per row, in LDS: KNN_SLOTS u64 keys, slots [0, 32) the
// sorted best so far (+inf keys at the start), slots [32, 56) pending
// candidates. Each lane keeps its row's bound tau (the key in slot k - 1)
// and the pending count in registers, identical in the row's four lanes. Per
// 16-row step js a lane tests its four keys against tau; the survivors'
// positions in the pending area come from the four lanes' counts exchanged
// by shuffles (lower g first), not from an atomic. A row whose pending area
// cannot take the step's keys (at most 16) is flushed first: the 64 lanes
// take one slot each, rank their key among the k best and the pending ones
// by broadcast reads (ties, which only the +inf keys have, go to the lower
// slot), and the ranks below k are written back in order; slots [k, 32) stay
// +inf. tau falls quickly: past the first tiles a whole wave usually has no
// survivor and skips everything after the compare.
//
// The order is that of the u64 key throughout, so equal distances go to the
// lower j, and the result does not depend on cols_per_block or on timing.
// Every block writes its rows' sorted k keys to part[y][i][0 .. k);
// knn_merge_kernel (one wave per row) merges the splits' lists.
// ---------------------------------------------------------------------------

#define KNN_BLOCK 256
#define KNN_TILE 64        // batch rows of a block; reference rows of a step
#define KNN_DC 64          // d-chunk staged in LDS
#define KNN_ZLD 68         // LDS row stride of a z tile (floats), as MMD_ZLD
#define KNN_MAX_K 32
#define KNN_SLOTS 56       // per row: KNN_MAX_K best, then the pending keys
#define KNN_PENDING (KNN_SLOTS - KNN_MAX_K)  // >= 16, what one step can add
#define KNN_MAX_ROWS 16384
#define KNN_MAX_SPLITS (KNN_MAX_ROWS / KNN_TILE)  // 4 list heads per merge lane
#define KNN_MAX_DP 4096
#define KNN_INF_KEY 0x7f800000ffffffffull  // d2 = +inf, j = -1

typedef unsigned long long knn_key;

// Orders a wave's LDS traffic: LDS serves one wave's instructions in issue
// order, so all that is needed is that the compiler keeps that order.
__device__ __forceinline__ void knn_wave_sync()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Sorts row `row` of the wave (uniform): slots [0, 32) and `pending` more.
// Returns the key of slot k - 1 afterwards. Called by all 64 lanes.
__device__ __forceinline__ knn_key knn_flush_row(knn_key* __restrict__ keys,
                                                 int pending, int k, int lane)
{
  // slots [k, 32) are never written: they hold +inf and are left out
  const bool live = lane < k || (lane >= KNN_MAX_K && lane < KNN_MAX_K + pending);
  const knn_key mine = live ? keys[lane] : KNN_INF_KEY;
  int rank = 0;
#pragma unroll
  for (int part = 0; part < 2; ++part) {
    const int lo = part ? KNN_MAX_K : 0, hi = part ? KNN_MAX_K + pending : k;
    for (int m0 = lo; m0 < hi; m0 += 8) {  // uniform; eight broadcast reads in flight
      knn_key other[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) other[u] = keys[min(m0 + u, hi - 1)];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int m = m0 + u;
        rank += (m < hi && (other[u] < mine || (other[u] == mine && m < lane))) ? 1 : 0;
      }
    }
  }
  knn_wave_sync();  // every read is done before a slot changes
  if (live && rank < k) keys[rank] = mine;
  knn_wave_sync();
  return keys[k - 1];
}

MMD_NO_PACKED_F32 __global__ __launch_bounds__(KNN_BLOCK) void knn_topk_kernel(
    const float* __restrict__ zb,       // [B, Dp] batch rows
    const float* __restrict__ zr,       // [M, Dp] reference rows
    const float* __restrict__ norms_b,  // [B]
    const float* __restrict__ norms_r,  // [Mp], 0 past M
    knn_key* __restrict__ part,         // [splits, rows, k]
    int B, int M, int Dp, int k, int cols_per_block, int row0, int rows,
    int exclude_self)
{
  __shared__ __attribute__((aligned(16))) float zi_s[KNN_TILE * KNN_ZLD];
  __shared__ __attribute__((aligned(16))) float zj_s[KNN_TILE * KNN_ZLD];
  __shared__ knn_key keys_s[KNN_TILE * KNN_SLOTS];

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int h = lane & 15, g = lane >> 4;
  const int i_base = row0 + (int)blockIdx.x * KNN_TILE;
  const int my_i = i_base + wave * 16 + h;
  const int j_begin = (int)blockIdx.y * cols_per_block;
  const int j_end = min(j_begin + cols_per_block, M);
  const bool i_ok = my_i < B && my_i < row0 + rows;
  const float n_i = norms_b[min(my_i, B - 1)];
  const int self_j = exclude_self ? my_i : -1;
  const int ld_c = tid & 15, ld_r = tid >> 4;
  const bool zi_once = Dp <= KNN_DC;
  knn_key* const wave_keys = keys_s + wave * 16 * KNN_SLOTS;
  knn_key* const my_keys = wave_keys + h * KNN_SLOTS;

  // the wave's own 16 x 32 best slots start at +inf
  for (int e = lane; e < 16 * KNN_MAX_K; e += 64)
    wave_keys[(e >> 5) * KNN_SLOTS + (e & 31)] = KNN_INF_KEY;
  knn_wave_sync();
  knn_key tau = KNN_INF_KEY;  // of row h; the same in its four lanes
  int pending = 0;            // likewise

  for (int j0 = j_begin; j0 < j_end; j0 += KNN_TILE) {
    mmd_f4 s[4];
#pragma unroll
    for (int js = 0; js < 4; ++js) s[js] = mmd_f4{0.f, 0.f, 0.f, 0.f};

    for (int d0 = 0; d0 < Dp; d0 += KNN_DC) {
      __syncthreads();  // the previous chunk (and tile) is consumed
      const int d = d0 + 4 * ld_c;  // Dp % 4 == 0: d < Dp covers d + 3
      const bool load_i = !zi_once || j0 == j_begin;  // uniform
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = ld_r + 16 * q;
        const int gi = i_base + row, gj = j0 + row;
        mmd_f4 vi = mmd_f4{0.f, 0.f, 0.f, 0.f}, vj = vi;
        if (load_i && d < Dp && gi < B)
          vi = *reinterpret_cast<const mmd_f4*>(zb + (size_t)gi * Dp + d);
        if (d < Dp && gj < M)
          vj = *reinterpret_cast<const mmd_f4*>(zr + (size_t)gj * Dp + d);
        if (load_i)
          *reinterpret_cast<mmd_f4*>(&zi_s[row * KNN_ZLD + 4 * ld_c]) = vi;
        *reinterpret_cast<mmd_f4*>(&zj_s[row * KNN_ZLD + 4 * ld_c]) = vj;
      }
      __syncthreads();

#pragma unroll
      for (int kk = 0; kk < KNN_DC / 16; ++kk) {
        if (d0 + kk * 16 >= Dp) continue;  // uniform
        const mmd_f4 b = *reinterpret_cast<const mmd_f4*>(
            &zi_s[(wave * 16 + h) * KNN_ZLD + kk * 16 + 4 * g]);
#pragma unroll
        for (int js = 0; js < 4; ++js) {
          const mmd_f4 a = *reinterpret_cast<const mmd_f4*>(
              &zj_s[(js * 16 + h) * KNN_ZLD + kk * 16 + 4 * g]);
          s[js] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, s[js], 0, 0, 0);
          s[js] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, s[js], 0, 0, 0);
          s[js] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, s[js], 0, 0, 0);
          s[js] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, s[js], 0, 0, 0);
        }
      }
    }

    // selection on the accumulators: s[js][r] is (j = jr + r, i = my_i)
#pragma unroll
    for (int js = 0; js < 4; ++js) {
      const int jr = j0 + js * 16 + 4 * g;
      const mmd_f4 n_j = *reinterpret_cast<const mmd_f4*>(norms_r + jr);
      knn_key cand[4];
      int n_mine = 0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float d2 = fmaxf(n_i + n_j[r] - 2.0f * s[js][r], 0.0f);
        const knn_key key =
            ((knn_key)(__float_as_uint(d2) & 0x7fffffffu) << 32) | (unsigned)(jr + r);
        const bool keep = i_ok && jr + r < j_end && jr + r != self_j && key < tau;
        cand[r] = keep ? key : KNN_INF_KEY;
        n_mine += keep ? 1 : 0;
      }
      if (__ballot(n_mine > 0) != 0ull) {  // rarely, past the first tiles
        // counts of the row's four lanes, lower g first
        const int c0 = __shfl(n_mine, h), c1 = __shfl(n_mine, h + 16);
        const int c2 = __shfl(n_mine, h + 32), c3 = __shfl(n_mine, h + 48);
        const int added = c0 + c1 + c2 + c3;  // <= 16
        // rows whose pending area cannot take this step's keys are sorted
        // first (their survivors were tested against the older, larger tau:
        // more than needed, never fewer)
        unsigned todo =
            (unsigned)(__ballot(pending + added > KNN_PENDING) & 0xffffull);
        while (todo) {  // uniform
          const int row = __ffs(todo) - 1;
          todo &= todo - 1;
          const knn_key t =
              knn_flush_row(wave_keys + row * KNN_SLOTS, __shfl(pending, row), k, lane);
          if (h == row) { tau = t; pending = 0; }
        }
        int at = KNN_MAX_K + pending +
                 (g > 0 ? c0 : 0) + (g > 1 ? c1 : 0) + (g > 2 ? c2 : 0);
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (cand[r] != KNN_INF_KEY) my_keys[at++] = cand[r];
        pending += added;  // <= KNN_PENDING
        knn_wave_sync();
      }
    }
  }

  // what is still pending, then the block's sorted lists
  unsigned todo = (unsigned)(__ballot(pending > 0) & 0xffffull);
  while (todo) {
    const int row = __ffs(todo) - 1;
    todo &= todo - 1;
    knn_flush_row(wave_keys + row * KNN_SLOTS, __shfl(pending, row), k, lane);
  }
  knn_wave_sync();
  for (int e = lane; e < 16 * k; e += 64) {
    const int row = e / k, slot = e - row * k;
    const int gi = i_base + wave * 16 + row;
    if (gi < B && gi < row0 + rows)
      part[((size_t)blockIdx.y * rows + (gi - row0)) * k + slot] =
          wave_keys[row * KNN_SLOTS + slot];
  }
}

// One wave per row: merges the splits' sorted lists part[s][row][0 .. k) into
// the k smallest keys. A lane owns the lists s = lane, lane + 64, ... (at
// most four) and offers the smallest of their heads; the wave takes the
// smallest offer k times. Keys of real pairs are unique; only +inf repeats.
MMD_NO_PACKED_F32 __global__ __launch_bounds__(KNN_BLOCK) void knn_merge_kernel(
    const knn_key* __restrict__ part, float* __restrict__ d2,
    int* __restrict__ idx, int splits, int rows, int k)
{
  const int lane = threadIdx.x & 63;
  const int row = (int)blockIdx.x * (KNN_BLOCK / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;  // a whole wave
  int head[KNN_MAX_SPLITS / 64] = {0, 0, 0, 0};
  for (int t = 0; t < k; ++t) {
    knn_key best = KNN_INF_KEY;
    int from = -1;
#pragma unroll
    for (int q = 0; q < KNN_MAX_SPLITS / 64; ++q) {
      const int s = lane + 64 * q;
      if (s < splits && head[q] < k) {
        const knn_key v = part[((size_t)s * rows + row) * k + head[q]];
        if (v < best) { best = v; from = q; }
      }
    }
    knn_key low = best;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const knn_key o = __shfl_xor(low, m);
      low = o < low ? o : low;
    }
    if (low != KNN_INF_KEY && best == low) {  // one lane: the key is unique
#pragma unroll
      for (int q = 0; q < KNN_MAX_SPLITS / 64; ++q)
        if (q == from) head[q] += 1;
    }
    if (lane == 0) {
      d2[(size_t)row * k + t] = __uint_as_float((unsigned)(low >> 32));
      idx[(size_t)row * k + t] = (int)(unsigned)(low & 0xffffffffull);
    }
  }
}

// The k nearest reference rows of batch rows [row_begin, row_begin +
// row_count): (d2 f32[row_count, k], idx i32[row_count, k]) ascending in
// (d2, j). z_batch f32[B, Dp] and z_ref f32[M, Dp] with D zero-padded to a
// multiple of 4, norms the squared row norms. exclude_self leaves out the
// pair j == i (global row numbers; both sides must then have as many rows).
std::vector<torch::Tensor> knn_topk(torch::Tensor z_batch, torch::Tensor z_ref,
                                    torch::Tensor norms_batch, torch::Tensor norms_ref,
                                    int64_t k, bool exclude_self,
                                    int64_t cols_per_block, int64_t row_begin,
                                    int64_t row_count)
{
  TORCH_CHECK(z_batch.is_cuda() && z_batch.scalar_type() == torch::kFloat32 &&
              z_batch.dim() == 2 && z_batch.is_contiguous(),
              "z_batch must be a contiguous f32[B, Dp] GPU tensor");
  TORCH_CHECK(z_ref.is_cuda() && z_ref.device() == z_batch.device() &&
              z_ref.scalar_type() == torch::kFloat32 && z_ref.dim() == 2 &&
              z_ref.is_contiguous() && z_ref.size(1) == z_batch.size(1),
              "z_ref must be a contiguous f32[M, Dp] tensor on z_batch's GPU");
  const int64_t B = z_batch.size(0), M = z_ref.size(0), Dp = z_batch.size(1);
  TORCH_CHECK(B >= 1 && B <= KNN_MAX_ROWS, "batch rows out of range: ", B);
  TORCH_CHECK(M >= 1 && M <= KNN_MAX_ROWS, "reference rows out of range: ", M);
  TORCH_CHECK(Dp >= 4 && Dp % 4 == 0 && Dp <= KNN_MAX_DP,
              "Dp must be a multiple of 4 in [4, ", KNN_MAX_DP, "]");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(z_batch.data_ptr<float>()) % 16 == 0 &&
              reinterpret_cast<uintptr_t>(z_ref.data_ptr<float>()) % 16 == 0,
              "z_batch and z_ref must be 16-byte aligned (rows are read as float4)");
  TORCH_CHECK(norms_batch.is_cuda() && norms_batch.device() == z_batch.device() &&
              norms_batch.scalar_type() == torch::kFloat32 && norms_batch.dim() == 1 &&
              norms_batch.size(0) == B && norms_batch.is_contiguous(),
              "norms_batch must be a contiguous f32[B] tensor on z_batch's GPU");
  TORCH_CHECK(norms_ref.is_cuda() && norms_ref.device() == z_batch.device() &&
              norms_ref.scalar_type() == torch::kFloat32 && norms_ref.dim() == 1 &&
              norms_ref.size(0) == M && norms_ref.is_contiguous(),
              "norms_ref must be a contiguous f32[M] tensor on z_batch's GPU");
  TORCH_CHECK(!exclude_self || B == M,
              "exclude_self needs the same rows on both sides");
  TORCH_CHECK(k >= 1 && k <= KNN_MAX_K && k <= M - (exclude_self ? 1 : 0),
              "k must be in [1, ", KNN_MAX_K, "] and at most the number of "
              "reference rows a batch row can take");
  TORCH_CHECK(cols_per_block >= KNN_TILE && cols_per_block % KNN_TILE == 0,
              "cols_per_block must be a positive multiple of ", KNN_TILE);
  if (row_count < 0) row_count = B - row_begin;
  TORCH_CHECK(row_begin >= 0 && row_begin % KNN_TILE == 0 && row_count >= 1 &&
              row_begin + row_count <= B,
              "row slice must start on a tile and lie inside [0, B)");

  c10::hip::HIPGuard guard((c10::DeviceIndex)z_batch.get_device());
  const int64_t Mp = (M + KNN_TILE - 1) / KNN_TILE * KNN_TILE;
  const int64_t splits = (M + cols_per_block - 1) / cols_per_block;  // <= 256
  // the kernel reads whole float4s of the reference norms unchecked
  auto norms_p = torch::zeros({Mp}, norms_ref.options());
  norms_p.slice(0, 0, M).copy_(norms_ref);
  auto part = torch::empty({splits, row_count, k}, z_batch.options().dtype(torch::kInt64));
  auto d2 = torch::empty({row_count, k}, z_batch.options());
  auto idx = torch::empty({row_count, k}, z_batch.options().dtype(torch::kInt32));

  hipStream_t stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(knn_topk_kernel,
      dim3((unsigned)((row_count + KNN_TILE - 1) / KNN_TILE), (unsigned)splits),
      dim3(KNN_BLOCK), 0, stream,
      z_batch.data_ptr<float>(), z_ref.data_ptr<float>(),
      norms_batch.data_ptr<float>(), norms_p.data_ptr<float>(),
      reinterpret_cast<knn_key*>(part.data_ptr<int64_t>()), (int)B, (int)M, (int)Dp,
      (int)k, (int)cols_per_block, (int)row_begin, (int)row_count,
      exclude_self ? 1 : 0);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(knn_merge_kernel,
      dim3((unsigned)((row_count + KNN_BLOCK / 64 - 1) / (KNN_BLOCK / 64))),
      dim3(KNN_BLOCK), 0, stream,
      reinterpret_cast<const knn_key*>(part.data_ptr<int64_t>()),
      d2.data_ptr<float>(), idx.data_ptr<int>(), (int)splits, (int)row_count, (int)k);
  HIP_CHECK(hipGetLastError());
  return {d2, idx};
}

// ---------------------------------------------------------------------------
// Forest proximity (creditcore/proximity.py): c(i, j) = the number of trees in
// which batch row i and reference row j end in the same leaf, and per batch
// row the k reference rows in the order (c descending, j ascending). Neither
// the B x M count matrix nor a one-hot over (tree, leaf) is ever held; the
// matrix cores have no part in it (leaf equality is not a bilinear form over
// a small alphabet).
//
//   forest_leaf_kernel       leaf[r, t] = absolute node index of the leaf row
//                            r reaches in tree t (both sides use it)
//   host (ops/gpu.py)        inverted index of the reference's leaf table:
//                            leaf_start[n_nodes + 1] (CSR by node index) and
//                            leaf_rows (the reference rows of each leaf, u16)
//   forest_prox_topk_kernel  one block per batch row: counts by walking the
//                            T row lists of its leaves, then a counting select
// ---------------------------------------------------------------------------

// Work split as forest_whatif_kernel: one thread owns a row, one wave per
// block, rows staged column-major in LDS with fused imputation (own slots
// only, so no barrier and threads past the last row leave at once).
// blockIdx.y picks a chunk of trees_per_chunk consecutive trees; LEAF_ILP of
// them are in flight per thread. Every entry of leaf[R, T] is written by a
// plain store.
//
// Bounds by construction (the note on forest_ale_kernel): a tree whose
// [base, base + size) does not lie inside the node table is skipped, a node
// index is compared unsigned against the tree's size before every load,
// source columns are clamped and the walk loop runs at most `size` times. A
// skipped tree, a bad child index, a feature index outside the table and a
// walk the loop bound stopped on a split all write -1, which
// forest_prox_topk_kernel never counts.
#define LEAF_BLOCK 64
#define LEAF_ILP 4

__global__ __launch_bounds__(LEAF_BLOCK) void forest_leaf_kernel(
    const short* __restrict__ codes,    // [R, N_CAT]
    const float* __restrict__ nums,     // [R, N_NUM], NaNs not yet imputed
    const float* __restrict__ medians,  // [N_NUM]
    const int4* __restrict__ nodes,     // [n_nodes] {feat, bits, left, right}
    const int* __restrict__ tree_off,   // [T+1]
    int n_trees,
    unsigned n_nodes,
    const int* __restrict__ feat_col,   // [F]
    const int* __restrict__ feat_code,  // [F]
    unsigned n_feat,
    int n_rows,
    int trees_per_chunk,
    int* __restrict__ leaf)             // [R, T]; every entry is written
{
  __shared__ short s_codes[N_CAT * LEAF_BLOCK];
  __shared__ float s_nums[N_NUM * LEAF_BLOCK];

  const int tid = threadIdx.x;
  const int row = blockIdx.x * LEAF_BLOCK + tid;
  if (row >= n_rows) return;  // no barrier below: own LDS slots only

#pragma unroll
  for (int c = 0; c < N_CAT; ++c)
    s_codes[c * LEAF_BLOCK + tid] = codes[(size_t)row * N_CAT + c];
#pragma unroll
  for (int c = 0; c < N_NUM; ++c) {
    const float v = nums[(size_t)row * N_NUM + c];
    s_nums[c * LEAF_BLOCK + tid] = isnan(v) ? medians[c] : v;
  }

  const int4 dead = make_int4(-1, 0, 0, 0);
  const int t_begin = blockIdx.y * trees_per_chunk;
  const int t_end = min(t_begin + trees_per_chunk, n_trees);
  int* __restrict__ out = leaf + (size_t)row * n_trees;

  for (int t = t_begin; t < t_end; t += LEAF_ILP) {
    int4 nd[LEAF_ILP];
    int base[LEAF_ILP], cur[LEAF_ILP];
    unsigned size[LEAF_ILP];
    unsigned longest = 0;
#pragma unroll
    for (int s = 0; s < LEAF_ILP; ++s) {
      base[s] = 0;
      size[s] = 0;
      cur[s] = -1;
      nd[s] = dead;
      if (t + s < t_end) {
        const int b0 = tree_off[t + s];
        const int sz = tree_off[t + s + 1] - b0;
        if (b0 >= 0 && sz > 0 && (unsigned)b0 + (unsigned)sz <= n_nodes) {
          base[s] = b0;
          size[s] = (unsigned)sz;
          cur[s] = b0;
          nd[s] = nodes[b0];
        }
      }
      longest = max(longest, size[s]);
    }
    bool any = true;
    for (unsigned it = 0; it < longest && any; ++it) {
      any = false;
#pragma unroll
      for (int s = 0; s < LEAF_ILP; ++s) {
        if ((unsigned)nd[s].x < n_feat) {
          const int fcol = feat_col[nd[s].x];
          const int code = feat_code[nd[s].x];
          const float v = (code >= 0)
              ? ((s_codes[min((unsigned)fcol, (unsigned)(N_CAT - 1)) * LEAF_BLOCK + tid] ==
                  (short)code) ? 1.0f : 0.0f)
              : s_nums[min((unsigned)fcol, (unsigned)(N_NUM - 1)) * LEAF_BLOCK + tid];
          const int rel = (v <= __int_as_float(nd[s].y)) ? nd[s].z : nd[s].w;
          if ((unsigned)rel < size[s]) {
            cur[s] = base[s] + rel;
            nd[s] = nodes[cur[s]];
          } else {
            cur[s] = -1;
            nd[s] = dead;
          }
          any = true;
        }
      }
    }
#pragma unroll
    for (int s = 0; s < LEAF_ILP; ++s)
      if (t + s < t_end) out[t + s] = (nd[s].x < 0) ? cur[s] : -1;
  }
}

// leaf i32[R, T] of the R rows in every classifier tree (forest_leaf_kernel).
// Stateless like forest_ale; the kernel bounds-checks the forest tables.
torch::Tensor forest_leaves(
    torch::Tensor codes, torch::Tensor nums,
    torch::Tensor cls_nodes, torch::Tensor cls_off,
    torch::Tensor feat_col, torch::Tensor feat_code,
    torch::Tensor medians, int64_t block_target)
{
  check_inputs(codes, nums);
  TORCH_CHECK(block_target >= 1 && block_target <= 65535, "bad block_target");
  auto on_dev = [&](const torch::Tensor& t, torch::ScalarType st, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.device() == codes.device(), name,
                " must be on the inputs' GPU");
    TORCH_CHECK(t.scalar_type() == st && t.is_contiguous(), name,
                " has the wrong dtype or is not contiguous");
  };
  on_dev(nums, torch::kFloat32, "nums");
  on_dev(cls_nodes, torch::kInt32, "cls_nodes");
  on_dev(cls_off, torch::kInt32, "cls_off");
  on_dev(feat_col, torch::kInt32, "feat_col");
  on_dev(feat_code, torch::kInt32, "feat_code");
  on_dev(medians, torch::kFloat32, "medians");
  TORCH_CHECK(cls_nodes.dim() == 2 && cls_nodes.size(1) == 4, "cls_nodes must be [n, 4]");
  TORCH_CHECK(cls_nodes.size(0) < (int64_t(1) << 31), "too many nodes");
  TORCH_CHECK(feat_col.numel() == feat_code.numel(), "feat_col/feat_code size mismatch");
  TORCH_CHECK(medians.numel() == N_NUM, "medians must have N_NUM entries");
  TORCH_CHECK(cls_off.dim() == 1 && cls_off.numel() >= 2, "forest has no trees");

  const int64_t R = codes.size(0);
  const int64_t T = cls_off.size(0) - 1;
  TORCH_CHECK(R >= 1, "forest_leaves needs at least one row");
  TORCH_CHECK(R * T < (int64_t(1) << 31), "too many (row, tree) pairs");

  c10::hip::HIPGuard guard((c10::DeviceIndex)codes.get_device());
  auto leaf = torch::empty({R, T},
      torch::TensorOptions().dtype(torch::kInt32).device(codes.device()));
  hipStream_t stream = c10::hip::getCurrentHIPStream();
  const int row_blocks = ceil_div((int)R, LEAF_BLOCK);
  // One-wave blocks; the trees are cut into chunks (whole LEAF_ILP groups)
  // until the grid has about block_target blocks.
  const int groups = ceil_div((int)T, LEAF_ILP);
  const int chunks = (int)std::max<int64_t>(
      1, std::min<int64_t>(ceil_div((int)block_target, row_blocks), groups));
  const int per_chunk = ceil_div(groups, chunks) * LEAF_ILP;
  hipLaunchKernelGGL(forest_leaf_kernel,
      dim3(row_blocks, ceil_div((int)T, per_chunk)), dim3(LEAF_BLOCK), 0, stream,
      codes.data_ptr<short>(), nums.data_ptr<float>(), medians.data_ptr<float>(),
      reinterpret_cast<const int4*>(cls_nodes.data_ptr<int>()),
      cls_off.data_ptr<int>(), (int)T, (unsigned)cls_nodes.size(0),
      feat_col.data_ptr<int>(), feat_code.data_ptr<int>(), (unsigned)feat_col.numel(),
      (int)R, per_chunk, leaf.data_ptr<int>());
  HIP_CHECK(hipGetLastError());
  return leaf;
}

// Counts and selection, one 256-thread block per batch row i.
//
// LDS (dynamic, sized by the launcher to M and T): the row's M counters as
// packed u16 pairs, ceil(M / 2) u32 (32 KiB at M = 16384), then T + 1
// histogram bins (16 KiB at T = 4096), zeroed by the block; PROX_MAX_K keys
// and three words of state are static. c <= T < 65536, so an add of 1 or of
// 1 << 16 never carries from the low half into the high one.
//
// Count phase. A group of lanes_per_tree lanes (a power of two, 1 to 64; the
// launcher picks it from the lengths of the lists a row meets) takes tree
// t = group, group + n_groups, ...: it reads the row's leaf id, the leaf's
// range in the index, and strides over the range, adding into the counter of
// every reference row listed. The adds are integer LDS atomics, so the counts
// do not depend on their order, on lanes_per_tree or on timing. Work per row
// is the number of co-memberships, sum_t |list of leaf_t|, not T x M. A leaf
// id outside [0, n_nodes) (the -1 of a skipped tree), a range outside the
// list and a row number outside [0, M) are dropped, not counted.
//
// Selection phase, a counting select:
//   1. histogram of the counter values over j (j == self left out); zeros,
//      which most counters hold, are added once per wave from a ballot;
//   2. wave 0 scans the bins downward from T, 64 at a time, for the largest
//      c* with #{j : c_j >= c*} >= k, and notes n_above = #{j : c_j > c*} < k;
//   3. every j with c_j > c* takes a key slot (LDS atomic, any order);
//   4. wave 0 scans j upward by ballot and takes the lowest j with
//      c_j == c* until k keys are held, then stops;
//   5. wave 0 ranks the k keys (T - c) << 14 | j (distinct, as j is) and
//      stores count[i, rank] and idx[i, rank].
// The launcher guarantees k <= M - exclude_self, so c* exists (zeros fill the
// list, lowest j first).
#define PROX_BLOCK 256
#define PROX_MAX_K 32
#define PROX_UNROLL 4         // list entries a lane loads before it adds them
#define PROX_MAX_ROWS 16384  // 14-bit j in the key, u16 in leaf_rows
#define PROX_MAX_TREES 4096   // (T - c) << 14 stays inside 27 bits

// Counter j of the packed pairs; never above T on a sound index, and clamped
// so that a bad one cannot leave the histogram or the key's bit field.
__device__ __forceinline__ unsigned prox_count_of(const unsigned* cnt, int j, int n_trees) {
  return min((cnt[j >> 1] >> ((j & 1) << 4)) & 0xffffu, (unsigned)n_trees);
}

__global__ __launch_bounds__(PROX_BLOCK) void forest_prox_topk_kernel(
    const int* __restrict__ leaf_batch,            // [B, T]
    const int* __restrict__ leaf_start,            // [n_nodes + 1]
    const unsigned short* __restrict__ leaf_rows,  // [n_list]
    unsigned n_nodes,
    int n_list,
    int n_trees,
    int n_ref,          // M
    int k,
    int lanes_per_tree,
    int row_begin,
    int exclude_self,
    int* __restrict__ count,  // [rows of the launch, k]; every entry is written
    int* __restrict__ idx)    // [rows of the launch, k]; every entry is written
{
  extern __shared__ unsigned prox_lds[];
  __shared__ unsigned s_keys[PROX_MAX_K];
  __shared__ int s_cstar, s_above, s_held;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int i = row_begin + blockIdx.x;
  const int self = exclude_self ? i : -1;
  const int n_pairs = (n_ref + 1) >> 1;
  unsigned* cnt = prox_lds;             // [n_pairs]
  unsigned* hist = prox_lds + n_pairs;  // [n_trees + 1]

  for (int w = tid; w < n_pairs + n_trees + 1; w += PROX_BLOCK) prox_lds[w] = 0u;
  if (tid < PROX_MAX_K) s_keys[tid] = 0xffffffffu;
  if (tid == 0) {
    s_held = 0;
    s_cstar = 0;
    s_above = 0;
  }
  __syncthreads();

  // ---- count
  {
    const int sub = tid & (lanes_per_tree - 1);
    const int n_groups = PROX_BLOCK / lanes_per_tree;
    const int* __restrict__ mine = leaf_batch + (size_t)i * n_trees;
    for (int t = tid / lanes_per_tree; t < n_trees; t += n_groups) {
      const int lf = mine[t];
      if ((unsigned)lf >= n_nodes) continue;
      const int p0 = leaf_start[lf];
      const int p1 = min(leaf_start[lf + 1], n_list);
      if (p0 < 0) continue;
      // PROX_UNROLL independent loads in flight per lane, then their adds: a
      // long list is bound by the latency of its 2-byte loads otherwise
      for (int p = p0 + sub; p < p1; p += PROX_UNROLL * lanes_per_tree) {
        unsigned j[PROX_UNROLL];
#pragma unroll
        for (int u = 0; u < PROX_UNROLL; ++u) {
          const int q = p + u * lanes_per_tree;
          j[u] = (q < p1) ? (unsigned)leaf_rows[q] : 0xffffffffu;
        }
#pragma unroll
        for (int u = 0; u < PROX_UNROLL; ++u)
          if (j[u] < (unsigned)n_ref) atomicAdd(&cnt[j[u] >> 1], 1u << ((j[u] & 1u) << 4));
      }
    }
  }
  __syncthreads();

  // ---- 1. histogram of the counts (whole waves stay in the loop: ballot)
  for (int j0 = wave * 64; j0 < n_ref; j0 += PROX_BLOCK) {
    const int j = j0 + lane;
    const bool live = j < n_ref && j != self;
    const unsigned c = live ? prox_count_of(cnt, j, n_trees) : 0u;
    const unsigned long long zeros = __ballot(live && c == 0u);
    if (live && c != 0u) atomicAdd(&hist[c], 1u);
    if (lane == 0 && zeros) atomicAdd(&hist[0], (unsigned)__popcll(zeros));
  }
  __syncthreads();

  // ---- 2. c* and n_above
  if (wave == 0) {
    int above = 0;  // #{j : c_j > top of this step}, wave-uniform
    for (int top = n_trees; top >= 0; top -= 64) {
      const int c = top - lane;
      const int h = (c >= 0) ? (int)hist[c] : 0;
      int incl = h;  // inclusive scan over the lanes: bins top .. top - lane
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
      }
      const unsigned long long hit = __ballot(c >= 0 && above + incl >= k);
      if (hit) {
        const int first = __ffsll((long long)hit) - 1;
        if (lane == first) {
          s_cstar = c;
          s_above = above + incl - h;
        }
        break;
      }
      above += __shfl(incl, 63);
    }
  }
  __syncthreads();
  const unsigned cstar = (unsigned)s_cstar;
  const int n_above = s_above;

  // ---- 3. every j above c*
  if (n_above > 0) {
    for (int j = tid; j < n_ref; j += PROX_BLOCK) {
      const unsigned c = prox_count_of(cnt, j, n_trees);
      if (c > cstar && j != self) {
        const int pos = atomicAdd(&s_held, 1);
        if (pos < PROX_MAX_K) s_keys[pos] = (((unsigned)n_trees - c) << 14) | (unsigned)j;
      }
    }
  }
  __syncthreads();

  // ---- 4. the lowest j at c*
  if (wave == 0) {
    int held = n_above;  // wave-uniform
    for (int j0 = 0; j0 < n_ref && held < k; j0 += 64) {
      const int j = j0 + lane;
      const bool hit = j < n_ref && j != self && prox_count_of(cnt, j, n_trees) == cstar;
      const unsigned long long m = __ballot(hit);
      const int rank = __popcll(m & ((1ull << lane) - 1ull));
      if (hit && held + rank < k)
        s_keys[held + rank] = (((unsigned)n_trees - cstar) << 14) | (unsigned)j;
      held = min(held + (int)__popcll(m), k);
    }
  }
  __syncthreads();

  // ---- 5. order the k keys
  if (wave == 0 && lane < k) {
    const unsigned key = s_keys[lane];
    int rank = 0;
    for (int q = 0; q < k; ++q) rank += (s_keys[q] < key) ? 1 : 0;
    const size_t at = (size_t)blockIdx.x * k + rank;
    count[at] = n_trees - (int)(key >> 14);
    idx[at] = (int)(key & 0x3fffu);
  }
}

// The k reference rows that share most leaves with batch rows [row_begin,
// row_begin + row_count): (count i32[row_count, k], idx i32[row_count, k]) in
// the order (count descending, j ascending). leaf_batch i32[B, T] is
// forest_leaves of the batch; leaf_start i32[n_nodes + 1] and leaf_rows
// i16[n_list] (row numbers below 16384, read unsigned) the inverted index of
// forest_leaves of the M reference rows. exclude_self leaves out the pair
// j == i (global row numbers; the batch must then be the reference).
std::vector<torch::Tensor> forest_prox_topk(
    torch::Tensor leaf_batch, torch::Tensor leaf_start, torch::Tensor leaf_rows,
    int64_t n_ref, int64_t k, bool exclude_self, int64_t lanes_per_tree,
    int64_t row_begin, int64_t row_count)
{
  TORCH_CHECK(leaf_batch.is_cuda() && leaf_batch.scalar_type() == torch::kInt32 &&
              leaf_batch.dim() == 2 && leaf_batch.is_contiguous(),
              "leaf_batch must be a contiguous i32[B, T] GPU tensor");
  TORCH_CHECK(leaf_start.is_cuda() && leaf_start.device() == leaf_batch.device() &&
              leaf_start.scalar_type() == torch::kInt32 && leaf_start.dim() == 1 &&
              leaf_start.is_contiguous() && leaf_start.numel() >= 2,
              "leaf_start must be a contiguous i32[n_nodes + 1] tensor on leaf_batch's GPU");
  TORCH_CHECK(leaf_rows.is_cuda() && leaf_rows.device() == leaf_batch.device() &&
              leaf_rows.scalar_type() == torch::kInt16 && leaf_rows.dim() == 1 &&
              leaf_rows.is_contiguous(),
              "leaf_rows must be a contiguous i16[n_list] tensor on leaf_batch's GPU");
  const int64_t B = leaf_batch.size(0), T = leaf_batch.size(1), M = n_ref;
  TORCH_CHECK(B >= 1 && B <= PROX_MAX_ROWS, "batch rows out of range: ", B);
  TORCH_CHECK(M >= 1 && M <= PROX_MAX_ROWS, "reference rows out of range: ", M);
  TORCH_CHECK(T >= 1 && T <= PROX_MAX_TREES, "trees out of range: ", T);
  TORCH_CHECK(leaf_rows.numel() <= M * T, "leaf_rows is longer than M x T");
  TORCH_CHECK(!exclude_self || B == M, "exclude_self needs the same rows on both sides");
  TORCH_CHECK(k >= 1 && k <= PROX_MAX_K && k <= M - (exclude_self ? 1 : 0),
              "k must be in [1, ", PROX_MAX_K, "] and at most the number of "
              "reference rows a batch row can take");
  TORCH_CHECK(lanes_per_tree >= 1 && lanes_per_tree <= 64 &&
              (lanes_per_tree & (lanes_per_tree - 1)) == 0,
              "lanes_per_tree must be a power of two in [1, 64]");
  if (row_count < 0) row_count = B - row_begin;
  TORCH_CHECK(row_begin >= 0 && row_count >= 1 && row_begin + row_count <= B,
              "row slice must lie inside [0, B)");

  c10::hip::HIPGuard guard((c10::DeviceIndex)leaf_batch.get_device());
  auto opt = torch::TensorOptions().dtype(torch::kInt32).device(leaf_batch.device());
  auto count = torch::empty({row_count, k}, opt);
  auto idx = torch::empty({row_count, k}, opt);
  const size_t lds = sizeof(unsigned) * (size_t)((M + 1) / 2 + T + 1);  // <= 48 KiB + 4 B
  hipStream_t stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(forest_prox_topk_kernel, dim3((unsigned)row_count),
      dim3(PROX_BLOCK), lds, stream,
      leaf_batch.data_ptr<int>(), leaf_start.data_ptr<int>(),
      reinterpret_cast<const unsigned short*>(leaf_rows.data_ptr<int16_t>()),
      (unsigned)(leaf_start.numel() - 1), (int)leaf_rows.numel(), (int)T, (int)M, (int)k,
      (int)lanes_per_tree, (int)row_begin, exclude_self ? 1 : 0,
      count.data_ptr<int>(), idx.data_ptr<int>());
  HIP_CHECK(hipGetLastError());
  return {count, idx};
}

// ---------------------------------------------------------------------------
// ScoreSession — one replica's resident GPU state + a single-call scoring
// path. Owns the model buffers in HBM, a private HIP stream, device
// workspace and pinned staging, so one Python call per request performs:
//   pinned H2D -> zero accumulators -> forest x2 -> finalize -> drift -> D2H
// with no per-call torch dispatch or allocation (the Python-side hot loop
// was ~10x the kernel time). The GIL is released while waiting.
// ---------------------------------------------------------------------------

// Completion waits: hipStreamSynchronize/hipEventSynchronize block on the
// runtime's interrupt-driven wakeup, which costs tens of µs of wake
// latency per request — a large share of the ~60 µs/request host floor at
// microsecond kernel times. Serving processes own their core, so the
// default is a polling wait (hipStreamQuery granularity ~1-2 µs);
// CREDITCORE_BLOCK_SYNC=1 restores blocking waits for A/B or
// share-the-host deployments.
inline bool spin_sync_enabled() {
  static const bool on = (std::getenv("CREDITCORE_BLOCK_SYNC") == nullptr);
  return on;
}

inline void sync_stream(hipStream_t s) {
  if (spin_sync_enabled()) {
    hipError_t e;
    while ((e = hipStreamQuery(s)) == hipErrorNotReady) {}
    if (e != hipSuccess) HIP_CHECK(e);
  } else {
    HIP_CHECK(hipStreamSynchronize(s));
  }
}

inline void sync_event(hipEvent_t ev) {
  // Event waits run on the EPILOGUE thread concurrently with the main
  // thread's hipGraphLaunch: a hipEventQuery spin there hammers the HIP
  // runtime's internal locks and was measured to double the launch cost
  // (submit 51 -> 96 us at b=1024). Block by default; CREDITCORE_SPIN_EVENT=1
  // restores the spin for single-threaded callers.
  static const bool spin = (std::getenv("CREDITCORE_SPIN_EVENT") != nullptr);
  if (spin) {
    hipError_t e;
    while ((e = hipEventQuery(ev)) == hipErrorNotReady) {}
    if (e != hipSuccess) HIP_CHECK(e);
  } else {
    HIP_CHECK(hipEventSynchronize(ev));
  }
}

struct ScoreSession {
  torch::Tensor cls_nodes, cls_off, feat_col, feat_code, medians;
  torch::Tensor if_nodes, if_off, ref_sorted, rs_off, cat_off;
  torch::Tensor d_codes, d_nums, acc, outs, d_drift, d_ks_scratch;
  size_t drift_bytes = 0, drift_ksd_off = 0;  // [hist i32 | ksd f32] blob
  torch::Tensor pin_codes, pin_nums, pin_outs, pin_drift;
  torch::Tensor pin_hist, pin_ksd;  // typed views into pin_drift
  double if_denom{}, if_offset{}, if_threshold{};
  int cls_kind{};
  double cls_bias{};
  int64_t total_bins{}, t_cls{}, t_if{}, capacity{};
  int device_index{};
  hipStream_t stream{};
  hipStream_t stream2{};  // drift branch (runs parallel to the forests)
  hipEvent_t ev_fork{}, ev_join{};
  hipEvent_t ev_done[2]{};  // per-slot completion (async score)

  // raw slot pointers into the pinned buffers
  int16_t* p_codes(int s) { return pin_codes.data_ptr<int16_t>() + (size_t)s * capacity * N_CAT; }
  float* p_nums(int s) { return pin_nums.data_ptr<float>() + (size_t)s * capacity * N_NUM; }
  double* p_outs(int s) { return pin_outs.data_ptr<double>() + (size_t)s * 3 * capacity; }
  uint8_t* p_drift(int s) { return pin_drift.data_ptr<uint8_t>() + (size_t)s * drift_bytes; }
  int32_t* p_hist(int s) { return reinterpret_cast<int32_t*>(p_drift(s)); }
  float* p_ksd(int s) { return reinterpret_cast<float*>(p_drift(s) + drift_ksd_off); }
  int32_t* d_hist() { return reinterpret_cast<int32_t*>(d_drift.data_ptr<uint8_t>()); }
  float* d_ksd() { return reinterpret_cast<float*>(d_drift.data_ptr<uint8_t>() + drift_ksd_off); }

  ScoreSession(py::dict model, int64_t cap, int dev) : capacity(cap), device_index(dev) {
    c10::hip::HIPGuard guard((c10::DeviceIndex)dev);
    auto devopt = torch::TensorOptions().device(torch::kCUDA, dev);
    auto up_i32 = [&](const char* k) {
      return py::cast<torch::Tensor>(model[k]).to(devopt.dtype(torch::kInt32)).contiguous();
    };
    auto up_f32 = [&](const char* k) {
      return py::cast<torch::Tensor>(model[k]).to(devopt.dtype(torch::kFloat32)).contiguous();
    };
    cls_nodes = up_i32("cls_nodes");
    cls_off = up_i32("cls_tree_offsets");
    feat_col = up_i32("feat_col");
    feat_code = up_i32("feat_code");
    medians = up_f32("medians");
    if_nodes = up_i32("if_nodes");
    if_off = up_i32("if_tree_offsets");
    ref_sorted = up_f32("ref_sorted");
    rs_off = py::cast<torch::Tensor>(model["ref_sorted_offsets"])
                 .to(devopt.dtype(torch::kInt64)).contiguous();
    cat_off = up_i32("ref_cat_offsets");
    if (model.contains("cls_kind")) cls_kind = py::cast<int>(model["cls_kind"]);
    if (model.contains("cls_bias")) cls_bias = py::cast<double>(model["cls_bias"]);
    if_denom = py::cast<double>(model["if_denom"]);
    if_offset = py::cast<double>(model["if_offset"]);
    if_threshold = py::cast<double>(model["if_threshold"]);
    t_cls = cls_off.size(0) - 1;
    t_if = if_off.size(0) - 1;
    total_bins = py::cast<torch::Tensor>(model["ref_cat_offsets"])[-1].item<int64_t>();

    d_codes = torch::empty({capacity, N_CAT}, devopt.dtype(torch::kInt16));
    d_nums = torch::empty({capacity, N_NUM}, devopt.dtype(torch::kFloat32));
    // all-zero invariant: finalize_kernel re-zeros the rows it consumes,
    // so record() never needs a memset node for the accumulators
    acc = torch::zeros({2, capacity}, devopt.dtype(torch::kFloat64));
    outs = torch::empty({3, capacity}, devopt.dtype(torch::kFloat64));
    // drift outputs packed into one blob: [hist i32 | ksd f32] — both are
    // b-independent sizes, so one D2H covers the whole drift branch
    drift_ksd_off = (size_t)total_bins * sizeof(int32_t);
    drift_bytes = drift_ksd_off + (size_t)N_NUM * sizeof(float);
    d_drift = torch::empty({(int64_t)drift_bytes}, devopt.dtype(torch::kUInt8));
    // per-(column, block) partial maxima for the multi-block counting K-S
    d_ks_scratch = torch::empty({(int64_t)N_NUM * KS_MB_MAX_G},
                                devopt.dtype(torch::kFloat32));

    // two slots: step i's host epilogue reads slot i%2 while step i+1's
    // graph fills the other slot (pipelined serving/bench loops)
    auto pinned = torch::TensorOptions().pinned_memory(true);
    pin_codes = torch::empty({2, capacity, N_CAT}, pinned.dtype(torch::kInt16));
    pin_nums = torch::empty({2, capacity, N_NUM}, pinned.dtype(torch::kFloat32));
    pin_outs = torch::empty({2, 3, capacity}, pinned.dtype(torch::kFloat64));
    pin_drift = torch::empty({2, (int64_t)drift_bytes}, pinned.dtype(torch::kUInt8));
    pin_hist = pin_drift.slice(1, 0, (int64_t)drift_ksd_off).view(torch::kInt32);
    pin_ksd = pin_drift.slice(1, (int64_t)drift_ksd_off, (int64_t)drift_bytes)
                  .view(torch::kFloat32);

    auto rs = py::cast<torch::Tensor>(model["ref_sorted_offsets"]);
    auto rs_acc = rs.accessor<int32_t, 1>();
    for (int j = 0; j + 1 < rs.size(0); ++j)
      max_ref_len = std::max(max_ref_len, (int64_t)(rs_acc[j + 1] - rs_acc[j]));

    // opt in to >64 KiB dynamic LDS for every launched K-S instantiation:
    // record() launches ks_kernel_t<512> (b=16384 needs exactly 64 KiB of
    // dynamic LDS, at/over the historical default cap), and the standalone
    // drift_stats/ks_stats paths launch <256>.
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ks_kernel_t<256>),
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)KS_LDS_BYTES);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ks_kernel_t<512>),
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)KS_LDS_BYTES);
    (void)hipFuncSetAttribute(
        reinterpret_cast<const void*>(&ks_count_mb_kernel_t<512>),
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)KS_LDS_BYTES);

    HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    HIP_CHECK(hipStreamCreateWithFlags(&stream2, hipStreamNonBlocking));
    HIP_CHECK(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&ev_done[0], hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&ev_done[1], hipEventDisableTiming));
    HIP_CHECK(hipDeviceSynchronize());  // uploads above used torch's stream
  }

  ~ScoreSession() {
    if (stream) {
      (void)hipStreamSynchronize(stream);
      for (auto& kv : graphs) (void)hipGraphExecDestroy(kv.second);
      (void)hipStreamDestroy(stream);
      (void)hipStreamDestroy(stream2);
      (void)hipEventDestroy(ev_fork);
      (void)hipEventDestroy(ev_join);
      (void)hipEventDestroy(ev_done[0]);
      (void)hipEventDestroy(ev_done[1]);
    }
  }

  // Record the full scoring sequence for batch size b on `stream`.
  // Output layout (b-packed so one D2H covers all three): outs holds
  // proba[0:b] | iscore[b:2b] | outlier[2b:3b]; pin_outs mirrors it.
  //
  // Two-stream shape (round-1 tuned): the drift branch (histogram + K-S)
  // forks onto stream2 off the H2D copies and joins after the output
  // copy. Both forests run as ONE dual-grid launch (forest_kernel_dual)
  // so the iforest rides along with the classifier instead of
  // serializing after it; a 3-stream fork for the same effect was
  // measured SLOWER (extra cross-stream graph edges ≈ +20 µs/replay at
  // b=1024 — kernel_tuning.md).
  void record(int b, bool with_drift, int slot) {
    HIP_CHECK(hipMemcpyAsync(d_codes.data_ptr(), p_codes(slot),
        (size_t)b * N_CAT * sizeof(short), hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(d_nums.data_ptr(), p_nums(slot),
        (size_t)b * N_NUM * sizeof(float), hipMemcpyHostToDevice, stream));
    // fork point: the drift branch (stream2) depends only on the H2D
    // copies. At tiny batches the drift kernels are microseconds and the
    // fork/join event edges cost more graph-replay overhead than the
    // overlap saves — run the branch inline on `stream` instead.
    const bool fork_drift = with_drift && b > 64;
    hipStream_t sdrift = fork_drift ? stream2 : stream;
    if (fork_drift) {
      HIP_CHECK(hipEventRecord(ev_fork, stream));
      HIP_CHECK(hipStreamWaitEvent(stream2, ev_fork, 0));
    }
    double* acc_cls = acc.data_ptr<double>();
    double* acc_if = acc_cls + b;  // b-packed; all-zero by invariant

    const int row_blocks = ceil_div(b, BLOCK);
    // 2-tree-ILP traversal measured faster at every batch size
    // (bench/kernel_micro.py: -12% @1k rows, -42% @16k); grid-y covers
    // ceil(T/2) chunks, each thread walking trees t and t+n_chunks.
    auto chunks = [&](int64_t t) {
      return std::max(1, std::min(ceil_div(2048, row_blocks), (int)((t + 1) / 2)));
    };
    const int c_cls = chunks(t_cls);
    const int c_if = chunks(t_if);
    hipLaunchKernelGGL(forest_kernel_dual, dim3(row_blocks, c_cls + c_if),
        dim3(BLOCK), 0, stream,
        d_codes.data_ptr<short>(), d_nums.data_ptr<float>(), medians.data_ptr<float>(),
        reinterpret_cast<const int4*>(cls_nodes.data_ptr<int>()),
        cls_off.data_ptr<int>(), (int)t_cls,
        feat_col.data_ptr<int>(), feat_code.data_ptr<int>(),
        reinterpret_cast<const int4*>(if_nodes.data_ptr<int>()),
        if_off.data_ptr<int>(), (int)t_if, c_cls, b, acc_cls, acc_if);

    double* proba = outs.data_ptr<double>();
    hipLaunchKernelGGL(finalize_kernel, dim3(row_blocks), dim3(BLOCK), 0, stream,
        acc_cls, acc_if, b, cls_kind, 1.0 / (double)t_cls, cls_bias,
        if_denom, if_offset, if_threshold,
        proba, proba + b, proba + 2 * b);

    if (with_drift) {
      // Drift branch: when forked (b > 64) the K-S and categorical
      // histogram run on stream2 in parallel with the forest chain
      // (captured as parallel graph branches, joined after the output
      // copy); at tiny batches everything stays serial on `stream`.
      // small batches: one block overwrites the histogram (no memset node);
      // larger ones pre-zero + atomically accumulate across blocks
      const int hist_blocks = (b <= 2048) ? 1 : std::min(row_blocks, 1024);
      if (hist_blocks > 1)
        HIP_CHECK(hipMemsetAsync(d_hist(), 0, (size_t)total_bins * sizeof(int), sdrift));
      hipLaunchKernelGGL(cat_hist_kernel, dim3(hist_blocks), dim3(BLOCK),
          (size_t)total_bins * sizeof(int), sdrift,
          d_codes.data_ptr<short>(), b, cat_off.data_ptr<int>(), (int)total_bins,
          d_hist());
      if (b <= KS_COUNT_MAX_ROWS) {
        // O(B^2) counting path: no sort, no barrier chain (38.6 -> single-
        // digit us at b=1024; see profiles/kernel_tuning.md)
        const size_t smem = (size_t)std::max(b, 512 / 64) * sizeof(float);
        hipLaunchKernelGGL((ks_count_kernel_t<512>), dim3(N_NUM), dim3(512),
            smem, sdrift,
            d_nums.data_ptr<float>(), medians.data_ptr<float>(), N_NUM, b,
            ref_sorted.data_ptr<float>(), rs_off.data_ptr<int64_t>(), d_ksd());
      } else if (std::getenv("CREDITCORE_KS_BITONIC") != nullptr) {
        // round-1 path kept for A/B: one bitonic-sort block per column
        // (only n_cols of 256 CUs busy; 38.6 us at b=1024, 509 at 16k)
        int m_pow2 = 512 / 64;  // >= one cross-wave reduction slot per wave
        while (m_pow2 < b) m_pow2 <<= 1;
        // measured (bench/kernel_micro.py on MI355X): staging the ref
        // column in LDS is slower at b=1024 (62 vs 48 us) and within noise
        // at 16k, so the ref stays in L2 (ref_lds=0).
        // 512 threads: halves the bitonic's serial depth per thread
        // (kernel_micro: 48.6->31.2 us @1k, 963->509 @16k)
        hipLaunchKernelGGL((ks_kernel_t<512>), dim3(N_NUM), dim3(512),
            (size_t)m_pow2 * sizeof(float), sdrift,
            d_nums.data_ptr<float>(), medians.data_ptr<float>(), N_NUM, b,
            m_pow2, /*ref_lds=*/0, ref_sorted.data_ptr<float>(),
            rs_off.data_ptr<int64_t>(), d_ksd());
      } else {
        // multi-block counting path: n_cols*g workgroups fill the chip
        // (the sort/count single-block kernels used 14 of 256 CUs)
        const int g = ks_mb_blocks(b);
        const size_t smem = (size_t)std::max(b, 512 / 64) * sizeof(float);
        hipLaunchKernelGGL((ks_count_mb_kernel_t<512>), dim3(N_NUM, g),
            dim3(512), smem, sdrift,
            d_nums.data_ptr<float>(), medians.data_ptr<float>(), N_NUM, b,
            ref_sorted.data_ptr<float>(), rs_off.data_ptr<int64_t>(),
            d_ks_scratch.data_ptr<float>());
        hipLaunchKernelGGL(ks_count_reduce_kernel, dim3(1), dim3(64), 0,
            sdrift, d_ks_scratch.data_ptr<float>(), g, N_NUM, d_ksd());
      }
      // one D2H for the whole drift branch (hist + K-S D share a blob)
      HIP_CHECK(hipMemcpyAsync(p_drift(slot), d_drift.data_ptr<uint8_t>(),
          drift_bytes, hipMemcpyDeviceToHost, sdrift));
      if (fork_drift) HIP_CHECK(hipEventRecord(ev_join, sdrift));
    }
    // classifier-output D2H depends only on finalize — it overlaps the
    // drift branch's K-S tail; the join lands after it so graph completion
    // still covers both streams
    HIP_CHECK(hipMemcpyAsync(p_outs(slot), proba,
        (size_t)(3 * b) * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (fork_drift) HIP_CHECK(hipStreamWaitEvent(stream, ev_join, 0));
    HIP_CHECK(hipGetLastError());
  }

  // Score b rows already staged in pin_codes/pin_nums. Blocks (GIL
  // released) until pin_outs/pin_hist/pin_ksd hold the results. The whole
  // sequence is captured into a hipGraph per (b, with_drift) and replayed
  // as one submit on subsequent requests of the same shape.
  void score(int64_t b64, bool with_drift, bool sync, int64_t slot64) {
    TORCH_CHECK(b64 >= 1 && b64 <= capacity, "batch out of range: ", b64);
    TORCH_CHECK(!with_drift || b64 <= MAX_DRIFT_ROWS, "drift batch too large: ", b64);
    TORCH_CHECK(slot64 == 0 || slot64 == 1, "slot must be 0/1");
    const int b = (int)b64;
    const int slot = (int)slot64;
    py::gil_scoped_release nogil;
    c10::hip::HIPGuard guard((c10::DeviceIndex)device_index);

    const uint64_t key = ((uint64_t)b << 2) | ((with_drift ? 1u : 0u) << 1) | (uint64_t)slot;
    // Only capture graphs for recurring shapes (powers of two and
    // 256-multiples — what the micro-batcher and bench produce). Arbitrary
    // merged sizes run the eager path directly: a capture costs ~ms, an
    // eager pass costs ~30 µs extra — capture churn would swamp the win.
    const bool graphable = ((b & (b - 1)) == 0) || (b % 256 == 0);
    auto it = graphs.find(key);
    if (it == graphs.end()) {
      if (!graphable || graphs.size() >= 128) {
        record(b, with_drift, slot);
        if (sync) sync_stream(stream);
        else HIP_CHECK(hipEventRecord(ev_done[slot], stream));
        return;
      }
      hipGraph_t graph;
      HIP_CHECK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
      record(b, with_drift, slot);
      HIP_CHECK(hipStreamEndCapture(stream, &graph));
      hipGraphExec_t exec;
      HIP_CHECK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
      HIP_CHECK(hipGraphDestroy(graph));
      it = graphs.emplace(key, exec).first;
    }
    HIP_CHECK(hipGraphLaunch(it->second, stream));
    if (sync) sync_stream(stream);
    else HIP_CHECK(hipEventRecord(ev_done[slot], stream));
  }

  void wait_slot(int64_t slot) {
    py::gil_scoped_release nogil;
    sync_event(ev_done[slot & 1]);
  }

  std::unordered_map<uint64_t, hipGraphExec_t> graphs;
  int64_t max_ref_len{};
  static constexpr size_t KS_LDS_BYTES = KS_LDS_BYTES_MAX;

  void synchronize() {
    py::gil_scoped_release nogil;
    HIP_CHECK(hipStreamSynchronize(stream));
  }
};

// ---------------------------------------------------------------------------
// Host-side request encoder (the native data-loader for the serving path).
// Replaces the reference's pandas DataFrame construction + sklearn
// OneHotEncoder lookup per request (reference app/main.py:54 →
// ColumnTransformer at 01-train cell-6) with one C pass over the parsed
// request dicts: ~20 µs per 1024-row request vs ~2 ms in Python.
// ---------------------------------------------------------------------------

#include <pybind11/numpy.h>

#include <cmath>
#include <string>
#include <unordered_map>
#include <vector>

namespace py = pybind11;

py::tuple encode_records(py::list recs, py::list vocabs, py::list cat_names,
                         py::list num_names, py::str missing_cat) {
  const ssize_t b = py::len(recs);
  const int ncat = (int)py::len(cat_names);
  const int nnum = (int)py::len(num_names);
  py::array_t<int16_t> codes({b, (ssize_t)ncat});
  py::array_t<float> nums({b, (ssize_t)nnum});
  auto* cp = codes.mutable_data();
  auto* fp = nums.mutable_data();

  std::vector<std::unordered_map<std::string, int16_t>> maps(ncat);
  std::vector<int16_t> missing_code(ncat, -1);
  const std::string miss = py::cast<std::string>(missing_cat);
  for (int j = 0; j < ncat; ++j) {
    py::list v = vocabs[j];
    for (ssize_t k = 0; k < py::len(v); ++k)
      maps[j][py::cast<std::string>(v[k])] = (int16_t)k;
    auto it = maps[j].find(miss);
    if (it != maps[j].end()) missing_code[j] = it->second;
  }
  std::vector<PyObject*> ckeys(ncat), nkeys(nnum);  // borrowed refs
  for (int j = 0; j < ncat; ++j) ckeys[j] = PyList_GET_ITEM(cat_names.ptr(), (ssize_t)j);
  for (int j = 0; j < nnum; ++j) nkeys[j] = PyList_GET_ITEM(num_names.ptr(), (ssize_t)j);

  for (ssize_t i = 0; i < b; ++i) {
    PyObject* r = PyList_GET_ITEM(recs.ptr(), i);
    if (!PyDict_Check(r)) throw py::type_error("record must be a dict");
    for (int j = 0; j < ncat; ++j) {
      PyObject* v = PyDict_GetItem(r, ckeys[j]);  // borrowed, NULL if absent
      int16_t code;
      if (v == nullptr || v == Py_None) {
        code = missing_code[j];  // SimpleImputer fill_value="missing"
      } else if (PyUnicode_Check(v)) {
        Py_ssize_t len;
        const char* s = PyUnicode_AsUTF8AndSize(v, &len);
        auto it = maps[j].find(std::string(s, (size_t)len));
        // unknown category -> -1 (OneHotEncoder handle_unknown="ignore")
        code = (it == maps[j].end()) ? (int16_t)-1 : it->second;
      } else if (PyFloat_Check(v) && std::isnan(PyFloat_AS_DOUBLE(v))) {
        code = missing_code[j];  // pandas-style NaN missing marker
      } else {
        throw py::value_error("categorical field must be a string/None");
      }
      cp[i * ncat + j] = code;
    }
    for (int j = 0; j < nnum; ++j) {
      PyObject* v = PyDict_GetItem(r, nkeys[j]);
      float x;
      if (v == nullptr || v == Py_None) {
        x = NAN;  // imputed to the median inside the scoring kernel
      } else if (PyFloat_Check(v)) {
        x = (float)PyFloat_AS_DOUBLE(v);
      } else if (PyLong_Check(v)) {
        x = (float)PyLong_AsDouble(v);
      } else {
        throw py::value_error("numeric field must be a number/None");
      }
      fp[i * nnum + j] = x;
    }
  }
  return py::make_tuple(codes, nums);
}

// ---------------------------------------------------------------------------
// The JSON request parser (jsonenc::Parser, JsonEncoderState,
// parse_records_nogil), the response writer (append_double,
// write_response_json) and the drift p-value epilogue (drift_pvals_raw) are
// plain C++ in host_codec.h, which tests/host/codec_harness.cpp also
// compiles on its own under the host sanitizers. Below are the wrappers that
// take and return Python objects; the GIL is released during the parse.
// ---------------------------------------------------------------------------

#include "host_codec.h"

static JsonEncoderState make_json_encoder(py::list vocabs, py::list cat_names,
                                          py::list num_names, py::str missing_cat,
                                          py::array_t<int16_t> default_codes,
                                          py::array_t<float> default_nums) {
  const size_t ncat = py::len(cat_names), nnum = py::len(num_names);
  TORCH_CHECK((size_t)default_codes.size() == ncat && (size_t)default_nums.size() == nnum,
      "default row size mismatch");
  std::vector<std::vector<std::string>> vocab(ncat);
  std::vector<std::string> cats, numn;
  for (size_t j = 0; j < ncat; ++j) {
    cats.push_back(py::cast<std::string>(cat_names[j]));
    py::list v = vocabs[j];
    for (size_t k = 0; k < py::len(v); ++k)
      vocab[j].push_back(py::cast<std::string>(v[k]));
  }
  for (size_t j = 0; j < nnum; ++j)
    numn.push_back(py::cast<std::string>(num_names[j]));
  return JsonEncoderState(
      std::move(vocab), cats, numn, py::cast<std::string>(missing_cat),
      std::vector<int16_t>(default_codes.data(), default_codes.data() + ncat),
      std::vector<float>(default_nums.data(), default_nums.data() + nnum));
}

py::tuple encode_json_impl(const JsonEncoderState& st, py::bytes body) {
  const int ncat = st.ncat;
  const int nnum = st.nnum;
  char* data;
  ssize_t blen;
  if (PyBytes_AsStringAndSize(body.ptr(), &data, &blen) != 0)
    throw py::value_error("body must be bytes");
  std::vector<int16_t> codes;
  std::vector<float> nums;
  size_t b;
  {
    py::gil_scoped_release nogil;
    try {
      b = parse_records_nogil(st, data, blen, codes, nums);
    } catch (const jsonenc::Error& e) {
      py::gil_scoped_acquire gil;
      throw py::value_error(e.msg);
    }
  }

  py::array_t<int16_t> codes_arr({(ssize_t)b, (ssize_t)ncat});
  py::array_t<float> nums_arr({(ssize_t)b, (ssize_t)nnum});
  if (b) {
    std::memcpy(codes_arr.mutable_data(), codes.data(), b * ncat * sizeof(int16_t));
    std::memcpy(nums_arr.mutable_data(), nums.data(), b * nnum * sizeof(float));
  }
  return py::make_tuple(codes_arr, nums_arr);
}

py::array_t<double> drift_pvals_host(
    py::array_t<int32_t> batch_hist, py::array_t<float> ks_d,
    py::array_t<int32_t> ref_cat_counts, py::array_t<int32_t> cat_offsets,
    int64_t n_ref, int64_t n_batch) {
  const int ncat = (int)cat_offsets.size() - 1;
  const int nnum = (int)ks_d.size();
  py::array_t<double> out({(ssize_t)(ncat + nnum)});
  drift_pvals_raw(batch_hist.data(), ks_d.data(), nnum, ref_cat_counts.data(),
                  cat_offsets.data(), ncat, n_ref, n_batch, out.mutable_data());
  return out;
}

py::tuple encode_json(py::bytes body, py::list vocabs, py::list cat_names,
                      py::list num_names, py::str missing_cat,
                      py::array_t<int16_t> default_codes,
                      py::array_t<float> default_nums) {
  const JsonEncoderState st = make_json_encoder(
      vocabs, cat_names, num_names, missing_cat, default_codes, default_nums);
  return encode_json_impl(st, body);
}

py::bytes build_response_json(py::object pin_outs, int64_t b,
                              py::array_t<double> pvals, py::list feature_names) {
  auto outs = py::cast<torch::Tensor>(pin_outs);
  const double* base = outs.data_ptr<double>();
  const double* proba = base;
  const double* outlier = base + 2 * b;
  const int nf = (int)py::len(feature_names);
  const double* pv = pvals.data();

  std::vector<std::string> names(nf);
  for (int j = 0; j < nf; ++j) names[j] = py::cast<std::string>(feature_names[j]);

  std::string out;
  {
    py::gil_scoped_release nogil;
    write_response_json(out, proba, outlier, b, pv, names);
  }
  return py::bytes(out);
}

// Serialize a /score response from plain arrays (the micro-batcher's
// merged-flush slices) — same wire bytes as build_response_json but not
// tied to the session's pinned layout. GIL released during the build.
py::bytes build_response_json_arrays(py::array_t<double> predictions,
                                     py::array_t<double> outliers,
                                     py::array_t<double> pvals,
                                     py::list feature_names) {
  const double* proba = predictions.data();
  const double* outl = outliers.data();
  const double* pv = pvals.data();
  const int64_t b = (int64_t)predictions.size();
  TORCH_CHECK((int64_t)outliers.size() == b, "outliers size mismatch");
  const int nf = (int)py::len(feature_names);
  TORCH_CHECK((int)pvals.size() == nf, "pvals size mismatch");
  std::vector<std::string> names(nf);
  for (int j = 0; j < nf; ++j) names[j] = py::cast<std::string>(feature_names[j]);

  std::string out;
  {
    py::gil_scoped_release nogil;
    write_response_json(out, proba, outl, b, pv, names);
  }
  return py::bytes(out);
}

// ---------------------------------------------------------------------------
// The consolidated request path: one call = parse wire JSON -> pinned
// staging -> graph replay -> drift p-values -> response JSON bytes. No
// Python object pass at any stage (GIL released around parse/serialize;
// ScoreSession::score releases it while waiting on the GPU).
// ---------------------------------------------------------------------------

py::tuple score_json_full(ScoreSession& s, py::bytes body,
                          const JsonEncoderState& st,
                          py::array_t<int32_t> ref_cat_counts,
                          py::array_t<int32_t> cat_offsets, int64_t n_ref,
                          py::list feature_names, int64_t drift_cap) {
  char* data;
  ssize_t blen;
  if (PyBytes_AsStringAndSize(body.ptr(), &data, &blen) != 0)
    throw py::value_error("body must be bytes");
  const int nf = (int)py::len(feature_names);
  TORCH_CHECK(nf == N_CAT + N_NUM, "feature name count mismatch");
  std::vector<std::string> names(nf);
  for (int j = 0; j < nf; ++j) names[j] = py::cast<std::string>(feature_names[j]);

  std::vector<int16_t> codes;
  std::vector<float> nums;
  size_t b;
  {
    py::gil_scoped_release nogil;
    try {
      b = parse_records_nogil(st, data, blen, codes, nums);
    } catch (const jsonenc::Error& e) {
      py::gil_scoped_acquire gil;
      throw py::value_error(e.msg);
    }
  }
  if (b == 0) throw py::value_error("empty request batch");
  TORCH_CHECK((int64_t)b <= s.capacity, "batch exceeds session capacity: ", b);

  std::memcpy(s.p_codes(0), codes.data(), b * N_CAT * sizeof(int16_t));
  std::memcpy(s.p_nums(0), nums.data(), b * N_NUM * sizeof(float));
  const int64_t cap = (drift_cap > 0) ? std::min<int64_t>(drift_cap, MAX_DRIFT_ROWS)
                                      : MAX_DRIFT_ROWS;
  int64_t nb = (int64_t)b;
  if ((int64_t)b <= cap) {
    s.score((int64_t)b, true, true, 0);
  } else {
    // Oversized batch: drift is a batch-population statistic, so run the
    // capped-sample drift pass FIRST (only with_drift passes write the
    // pinned drift region), then the full batch without drift — pin_outs
    // then holds the b-packed layout the serializer below reads. Running
    // the passes the other way round overwrote the b-packed outputs with a
    // cap-packed layout and corrupted rows >= cap (round-1 advisor
    // finding).
    s.score(cap, true, true, 0);
    s.score((int64_t)b, false, true, 0);
    nb = cap;
  }

  double pv[N_CAT + N_NUM];
  drift_pvals_raw(s.p_hist(0), s.p_ksd(0), N_NUM,
                  ref_cat_counts.data(), cat_offsets.data(),
                  (int)cat_offsets.size() - 1, n_ref, nb, pv);

  std::string out;
  {
    py::gil_scoped_release nogil;
    const double* proba = s.p_outs(0);
    const double* outlier = proba + 2 * b;
    write_response_json(out, proba, outlier, (int64_t)b, pv, names);
  }
  return py::make_tuple(py::bytes(out), (int64_t)b);
}

// Stage encoded arrays into a pinned slot and launch — one C call with
// the GIL released around the memcpys (the numpy slice-assign staging it
// replaces held the GIL for ~10 µs per step).
void submit_arrays(ScoreSession& s, py::array_t<int16_t> codes,
                   py::array_t<float> nums, int64_t slot, bool with_drift,
                   bool sync) {
  TORCH_CHECK(codes.ndim() == 2 && codes.shape(1) == N_CAT, "codes must be [B, N_CAT]");
  TORCH_CHECK(nums.ndim() == 2 && nums.shape(1) == N_NUM, "nums must be [B, N_NUM]");
  const int64_t b = codes.shape(0);
  TORCH_CHECK(nums.shape(0) == b, "codes/nums row mismatch");
  TORCH_CHECK(b >= 1 && b <= s.capacity, "batch out of range: ", b);
  auto c = codes.unchecked<2>();
  auto n = nums.unchecked<2>();
  const int sl = (int)(slot & 1);
  {
    py::gil_scoped_release nogil;
    // pybind returns row-contiguous for c_style-convertible inputs; copy
    // row-wise to stay correct for any stride
    int16_t* pc = s.p_codes(sl);
    float* pn = s.p_nums(sl);
    if (codes.strides(0) == (ssize_t)(N_CAT * sizeof(int16_t)) &&
        codes.strides(1) == (ssize_t)sizeof(int16_t)) {
      std::memcpy(pc, c.data(0, 0), (size_t)b * N_CAT * sizeof(int16_t));
    } else {
      for (int64_t i = 0; i < b; ++i)
        for (int j = 0; j < N_CAT; ++j) pc[i * N_CAT + j] = c(i, j);
    }
    if (nums.strides(0) == (ssize_t)(N_NUM * sizeof(float)) &&
        nums.strides(1) == (ssize_t)sizeof(float)) {
      std::memcpy(pn, n.data(0, 0), (size_t)b * N_NUM * sizeof(float));
    } else {
      for (int64_t i = 0; i < b; ++i)
        for (int j = 0; j < N_NUM; ++j) pn[i * N_NUM + j] = n(i, j);
    }
  }
  s.score(b, with_drift, sync, sl);
}

// Pipelined epilogue: wait for slot's graph, convert drift p-values and
// serialize the response from that slot's pinned buffers.
py::bytes response_epilogue(ScoreSession& s, int64_t slot64, int64_t b64,
                            py::array_t<int32_t> ref_cat_counts,
                            py::array_t<int32_t> cat_offsets, int64_t n_ref,
                            py::list feature_names) {
  const int slot = (int)slot64 & 1;
  const int64_t b = b64;
  TORCH_CHECK(b >= 1 && b <= s.capacity, "batch out of range: ", b);
  const int nf = (int)py::len(feature_names);
  std::vector<std::string> names(nf);
  for (int j = 0; j < nf; ++j) names[j] = py::cast<std::string>(feature_names[j]);
  const int64_t nb = std::min<int64_t>(b, MAX_DRIFT_ROWS);

  double pv[N_CAT + N_NUM];
  std::string out;
  {
    py::gil_scoped_release nogil;
    sync_event(s.ev_done[slot]);
    drift_pvals_raw(s.p_hist(slot), s.p_ksd(slot), N_NUM,
                    ref_cat_counts.data(), cat_offsets.data(),
                    (int)cat_offsets.size() - 1, n_ref, nb, pv);
    const double* proba = s.p_outs(slot);
    const double* outlier = proba + 2 * b;
    write_response_json(out, proba, outlier, b, pv, names);
  }
  return py::bytes(out);
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("score_forest_pipeline", &score_forest_pipeline,
        "Forest classifier + isolation forest scoring (gfx950)");
  m.def("forest_contrib", &forest_contrib,
        "Per-row prediction-path feature attributions f64[B,23] (gfx950)",
        py::arg("codes"), py::arg("nums"), py::arg("cls_nodes"),
        py::arg("cls_node_value"), py::arg("cls_off"), py::arg("feat_col"),
        py::arg("feat_code"), py::arg("medians"), py::arg("cls_kind"),
        py::arg("block_target") = 512);
  m.def("forest_shap", &forest_shap,
        "Per-row exact TreeSHAP feature attributions f64[B,23] (gfx950)",
        py::arg("codes"), py::arg("nums"), py::arg("leaf_value"),
        py::arg("leaf_off"), py::arg("splits"), py::arg("medians"),
        py::arg("cls_kind"), py::arg("n_trees"),
        py::arg("block_target") = 2048);
  m.def("forest_shap_interactions", &forest_shap_interactions,
        "Per-row exact SHAP interaction values f64[B,23,23], diagonal left "
        "at zero (gfx950)",
        py::arg("codes"), py::arg("nums"), py::arg("leaf_value"),
        py::arg("leaf_off"), py::arg("splits"), py::arg("medians"),
        py::arg("cls_kind"), py::arg("n_trees"),
        py::arg("block_target") = 2048);
  m.attr("SHAP_INTER_ROWS_PER_BLOCK") = py::int_(SHAPI_ROWS);
  m.def("forest_ishap", &forest_ishap,
        "Per-row interventional Shapley values f64[B,23] against a "
        "background sample (gfx950)",
        py::arg("codes"), py::arg("nums"), py::arg("bg_codes"),
        py::arg("bg_nums"), py::arg("leaf_value"), py::arg("leaf_off"),
        py::arg("splits"), py::arg("medians"), py::arg("cls_kind"),
        py::arg("n_trees"), py::arg("block_target") = 2048);
  m.attr("ISHAP_MAX_BACKGROUND") = py::int_(ISHAP_MAX_BACKGROUND);
  m.def("forest_whatif", &forest_whatif,
        "What-if raw forest sums f64[J,R]: every sample row under every "
        "job's one or two column overrides (partial dependence; gfx950)",
        py::arg("codes"), py::arg("nums"), py::arg("cls_nodes"),
        py::arg("cls_off"), py::arg("feat_col"), py::arg("feat_code"),
        py::arg("medians"), py::arg("jobs"), py::arg("block_target") = 8192);
  m.attr("WHATIF_ROWS_PER_BLOCK") = py::int_(WHATIF_BLOCK);
  m.def("forest_ale", &forest_ale,
        "Accumulated local effects: per (entry, row) the row's grid interval "
        "and the raw forest sums at its two edges, {i32[E,R], f64[E,R,2]} "
        "(dual walk; gfx950)",
        py::arg("codes"), py::arg("nums"), py::arg("cls_nodes"),
        py::arg("cls_off"), py::arg("feat_col"), py::arg("feat_code"),
        py::arg("medians"), py::arg("players"), py::arg("edge_off"),
        py::arg("edges"), py::arg("block_target") = 8192);
  m.attr("ALE_ROWS_PER_BLOCK") = py::int_(ALE_BLOCK);
  m.attr("ALE_MAX_EDGES") = py::int_(ALE_MAX_EDGES);
  m.def("forest_permute", &forest_permute,
        "Permutation importance: per (table row, sample row) the raw forest "
        "sum of the row with one column taken from its donor row, f64[Q,R] "
        "(shared base walk, the repeats of a feature side by side; gfx950)",
        py::arg("codes"), py::arg("nums"), py::arg("cls_nodes"),
        py::arg("cls_off"), py::arg("feat_col"), py::arg("feat_code"),
        py::arg("medians"), py::arg("perm_player"), py::arg("perm"),
        py::arg("block_target") = 8192);
  m.attr("PERM_ROWS_PER_BLOCK") = py::int_(PERM_BLOCK);
  m.attr("PERM_ILP") = py::int_(PERM_ILP);
  m.def("forest_anchor", &forest_anchor,
        "Anchor rules: per candidate anchor (a set of pinned features) of a "
        "row, the number of sample rows whose composite scores above cut, "
        "{i32[M], f64[M,S] with want_sums} (one walk of a tree serves all "
        "candidates of a chunk; gfx950)",
        py::arg("codes"), py::arg("nums"), py::arg("bg_codes"),
        py::arg("bg_nums"), py::arg("cls_nodes"), py::arg("cls_off"),
        py::arg("feat_col"), py::arg("feat_code"), py::arg("medians"),
        py::arg("sat"), py::arg("masks"), py::arg("mask_off"),
        py::arg("cut"), py::arg("want_sums") = false, py::arg("chunk") = 0,
        py::arg("block_target") = 4096);
  m.attr("ANCHOR_CHUNK") = py::int_(ANCHOR_CHUNK);
  m.def("forest_sweep", &forest_sweep,
        "Exact single-feature sweep: per {row, numeric column} job the raw "
        "forest sum of every threshold interval, searched on the device for "
        "the nearest decision flips (counterfactuals; gfx950)",
        py::arg("codes"), py::arg("nums"), py::arg("cls_nodes"),
        py::arg("cls_off"), py::arg("feat_col"), py::arg("feat_code"),
        py::arg("medians"), py::arg("node_rank"), py::arg("thr"),
        py::arg("thr_off"), py::arg("jobs"), py::arg("cut"),
        py::arg("max_depth"), py::arg("want_curves") = false);
  m.attr("SWEEP_BLOCK") = py::int_(SWEEP_BLOCK);
  m.attr("SWEEP_CHUNK") = py::int_(SWEEP_CHUNK);
  m.attr("SWEEP_SEG_CAP") = py::int_(SWEEP_SEG_CAP);
  m.attr("SWEEP_MAX_DEPTH") = py::int_(SWEEP_MAX_DEPTH);
  m.def("hgbt_hist", &hgbt_hist,
        "HistGBT level histogram i64[n_nodes,3,total_bins] of int32 "
        "fixed-point gradients (gfx950)",
        py::arg("bins"), py::arg("bin_off"), py::arg("grp_off"),
        py::arg("node"), py::arg("gq"), py::arg("hq"), py::arg("n_nodes"),
        py::arg("total_bins"), py::arg("lds_entries"),
        py::arg("rows_per_block") = HGBT_MAX_ROWS_PER_BLOCK);
  m.def("hgbt_split", &hgbt_split,
        "HistGBT best split per open node, i64[n_nodes,9] records (gfx950)",
        py::arg("hist"), py::arg("bin_off"), py::arg("lam"), py::arg("min_leaf"));
  m.def("hgbt_split_mono", &hgbt_split_mono,
        "HistGBT best split per open node under monotone constraints: feature "
        "signs i32[F], per-node weight bounds f64[n_nodes,2] (gfx950)",
        py::arg("hist"), py::arg("bin_off"), py::arg("lam"), py::arg("min_leaf"),
        py::arg("mono"), py::arg("bounds"));
  m.def("hgbt_route", &hgbt_route,
        "HistGBT: move rows to their child node or leaf, in place (gfx950)",
        py::arg("bins"), py::arg("table"), py::arg("node"));
  m.attr("HGBT_SHIFT") = py::int_(HGBT_SHIFT);
  m.attr("HGBT_MAX_ROWS_PER_BLOCK") = py::int_(HGBT_MAX_ROWS_PER_BLOCK);
  m.attr("HGBT_LDS_BYTES_MAX") = py::int_(HGBT_LDS_BYTES_MAX);
  m.def("bin_select", &bin_select,
        "Binning summary of the columns [f0, f1) of x f32[N,F] by multi-rank "
        "radix select -> {keys i32[G,N], state i64[G,BIN_ST_WORDS]} (gfx950)",
        py::arg("x"), py::arg("f0"), py::arg("f1"), py::arg("max_bins"),
        py::arg("launch_rows"));
  m.def("bin_assign", &bin_assign,
        "u8 bins of a column group from its keys and edge keys, written into "
        "bins[f0:f0+G] (gfx950)",
        py::arg("keys"), py::arg("edges"), py::arg("bins"), py::arg("f0"),
        py::arg("launch_rows"));
  m.attr("BIN_GROUP_COLS") = py::int_(BIN_GROUP_COLS);
  m.attr("BIN_SLOTS") = py::int_(BIN_SLOTS);
  m.def("hrf_hist", &hrf_hist,
        "HistForest level histogram i64[n_slots,2,total_bins] of a tree batch "
        "(gfx950)",
        py::arg("bins"), py::arg("bin_off"), py::arg("grp_off"), py::arg("y"),
        py::arg("w"), py::arg("node"), py::arg("slot_off"), py::arg("n_slots"),
        py::arg("total_bins"), py::arg("lds_entries"),
        py::arg("rows_per_block") = HRF_MAX_ROWS_PER_BLOCK);
  m.def("hrf_split", &hrf_split,
        "HistForest chosen split per open slot, i64[n_slots,7] records (gfx950)",
        py::arg("hist"), py::arg("bin_off"), py::arg("slot_meta"),
        py::arg("max_features"), py::arg("min_leaf"), py::arg("seed"));
  m.def("hrf_route", &hrf_route,
        "HistForest: move the rows of every tree of the batch, in place (gfx950)",
        py::arg("bins"), py::arg("table"), py::arg("node"), py::arg("slot_off"));
  m.def("hrf_seg_build", &hrf_seg_build,
        "HistForest segmented level: open rows bucketed by slot -> {seg_off, rows}",
        py::arg("bins"), py::arg("y"), py::arg("w"), py::arg("node"),
        py::arg("slot_off"), py::arg("n_slots"), py::arg("max_open"));
  m.def("hrf_seg_split", &hrf_seg_split,
        "HistForest segmented level: split record per open slot -> i64[n_slots, 7]",
        py::arg("rows"), py::arg("seg_off"), py::arg("bins_rm"), py::arg("bin_off"),
        py::arg("slot_meta"), py::arg("max_features"), py::arg("min_leaf"),
        py::arg("seed"));
  m.attr("HRF_SEG_CHUNK") = py::int_(HRF_SEG_CHUNK);
  m.attr("HRF_MAX_ROWS_PER_BLOCK") = py::int_(HRF_MAX_ROWS_PER_BLOCK);
  m.attr("HRF_MAX_FEATS") = py::int_(HRF_MAX_FEATS);
  m.def("drift_stats", &drift_stats,
        "Per-feature drift statistics: categorical histograms + K-S D (gfx950)");
  m.def("mmd_perm_w", &mmd_perm_w,
        "MMD permutation test: W = K . ind as f64[rows, Q], the RBF Gram "
        "matrix K fused away on the matrix cores (gfx950)",
        py::arg("z"), py::arg("norms"), py::arg("gamma"), py::arg("ind"),
        py::arg("cols_per_block"), py::arg("row_begin") = 0,
        py::arg("row_count") = -1);
  m.attr("MMD_TILE") = py::int_(MMD_TILE);
  m.def("knn_topk", &knn_topk,
        "k nearest reference rows per batch row -> (d2 f32[rows, k], idx "
        "i32[rows, k]): distance GEMM on the matrix cores fused with a "
        "running top-k, no distance matrix (gfx950)",
        py::arg("z_batch"), py::arg("z_ref"), py::arg("norms_batch"),
        py::arg("norms_ref"), py::arg("k"), py::arg("exclude_self"),
        py::arg("cols_per_block"), py::arg("row_begin") = 0,
        py::arg("row_count") = -1);
  m.def("forest_leaves", &forest_leaves,
        "leaf i32[R, T]: the absolute node index of the leaf every row reaches "
        "in every classifier tree, -1 for a tree outside the node table (gfx950)",
        py::arg("codes"), py::arg("nums"), py::arg("cls_nodes"),
        py::arg("cls_off"), py::arg("feat_col"), py::arg("feat_code"),
        py::arg("medians"), py::arg("block_target") = 2048);
  m.def("forest_prox_topk", &forest_prox_topk,
        "forest proximity: per batch row the k reference rows sharing most "
        "leaves -> (count i32[rows, k], idx i32[rows, k]) in the order (count "
        "desc, j asc); counts from an inverted leaf index in LDS u16 counters, "
        "counting select, no B x M array (gfx950)",
        py::arg("leaf_batch"), py::arg("leaf_start"), py::arg("leaf_rows"),
        py::arg("n_ref"), py::arg("k"), py::arg("exclude_self"),
        py::arg("lanes_per_tree") = 64, py::arg("row_begin") = 0,
        py::arg("row_count") = -1);
  m.attr("PROX_MAX_K") = py::int_(PROX_MAX_K);
  m.attr("PROX_MAX_TREES") = py::int_(PROX_MAX_TREES);
  m.attr("KNN_TILE") = py::int_(KNN_TILE);
  m.attr("KNN_MAX_K") = py::int_(KNN_MAX_K);
  m.def("encode_records", &encode_records,
        "Native request encoder: list[dict] -> (codes i16[B,9], nums f32[B,14])");
  m.def("encode_json", &encode_json,
        "Parse a /score JSON request body straight into (codes, nums)");
  py::class_<JsonEncoderState>(m, "JsonEncoder")
      .def(py::init(&make_json_encoder))
      .def("encode", [](const JsonEncoderState& st, py::bytes body) {
        return encode_json_impl(st, body);
      });
  m.def("dense_score", &dense_score,
        "Fused impute + logistic linear score + robust-z outlier (gfx950)");
  m.def("impute_transpose", &impute_transpose,
        "Fused NaN->median impute + transpose [B,F] -> [F,B] (gfx950)");
  m.def("ks_stats_sorted", &ks_stats_sorted,
        "Exact K-S D per column for pre-sorted batch columns (gfx950)");
  m.def("forest_ilp_bench", &forest_ilp_bench,
        "A/B: forest traversal, 1 vs 2 trees per thread");
  m.def("ks_stats", &ks_stats,
        "Exact two-sample K-S D per column, any column count (gfx950)",
        py::arg("nums"), py::arg("medians"), py::arg("ref_sorted"),
        py::arg("rs_off"), py::arg("block") = 256, py::arg("ref_lds") = 0);
  m.def("build_response_json", &build_response_json,
        "Serialize the /score response to JSON bytes (C, shortest doubles)");
  m.def("build_response_json_arrays", &build_response_json_arrays,
        "Serialize a /score response from plain arrays (merged-flush slices)");
  m.def("drift_pvals_host", &drift_pvals_host,
        "Drift p-values from kernel statistics (chi2 + Pelz-Good K-S), host C");
  py::class_<ScoreSession>(m, "ScoreSession")
      .def(py::init<py::dict, int64_t, int>(), py::arg("model"),
           py::arg("capacity"), py::arg("device_index"))
      .def("score", &ScoreSession::score, py::arg("b"),
           py::arg("with_drift") = true, py::arg("sync") = true,
           py::arg("slot") = 0)
      .def("wait_slot", &ScoreSession::wait_slot)
      .def("submit_arrays", &submit_arrays, py::arg("codes"), py::arg("nums"),
           py::arg("slot") = 0, py::arg("with_drift") = true,
           py::arg("sync") = false)
      .def("response_epilogue", &response_epilogue, py::arg("slot"),
           py::arg("b"), py::arg("ref_cat_counts"), py::arg("cat_offsets"),
           py::arg("n_ref"), py::arg("feature_names"))
      .def("synchronize", &ScoreSession::synchronize)
      .def("score_json_full", &score_json_full, py::arg("body"),
           py::arg("encoder"), py::arg("ref_cat_counts"),
           py::arg("cat_offsets"), py::arg("n_ref"), py::arg("feature_names"),
           py::arg("drift_cap") = -1)
      .def_readonly("capacity", &ScoreSession::capacity)
      .def_property_readonly("pin_codes", [](ScoreSession& s) { return s.pin_codes; })
      .def_property_readonly("pin_nums", [](ScoreSession& s) { return s.pin_nums; })
      .def_property_readonly("pin_outs", [](ScoreSession& s) { return s.pin_outs; })
      .def_property_readonly("pin_hist", [](ScoreSession& s) { return s.pin_hist; })
      .def_property_readonly("pin_ksd", [](ScoreSession& s) { return s.pin_ksd; });
}
