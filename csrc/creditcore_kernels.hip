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

// One block per open slot. Phase 1 (hgbt_split_kernel's scan): each wavefront
// takes every 4th feature, a lane owns 4 bins, and the feature's best valid
// split (highest proxy, lowest bin) goes to the LDS table. Phase 2: feature
// keys, ranks by (key, f), r* = lowest rank with a valid split, and among the
// ranks below max(max_features, r* + 1) the highest proxy, ties to the lower
// rank.
__global__ __launch_bounds__(HGBT_BLOCK) void hrf_split_kernel(
    const long long* __restrict__ hist, const int* __restrict__ bin_off,
    const int* __restrict__ slot_meta, int n_feat, int total_bins,
    int max_features, long long min_leaf, unsigned long long seed,
    long long* __restrict__ out)
{
  __shared__ double f_proxy[HRF_MAX_FEATS];
  __shared__ unsigned long long f_key[HRF_MAX_FEATS];
  __shared__ long long f_pl[HRF_MAX_FEATS], f_wl[HRF_MAX_FEATS];
  __shared__ int f_bin[HRF_MAX_FEATS];  // -1: the feature has no valid split
  __shared__ int f_rank[HRF_MAX_FEATS];
  __shared__ long long tot[2];
  __shared__ int r_star;
  __shared__ HrfPick wave_pick[HGBT_BLOCK / 64];
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
    double bp = 0.0;
    int bb = -1;
    long long bpl = 0, bwl = 0;
    if (!(fb < 0 || nb <= 0 || nb > HGBT_MAX_BINS || fb + nb > total_bins)) {
      long long pp[4], pw[4];
      long long sp = 0, sw = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int b = lane * 4 + j;
        if (b < nb) { sp += hp[fb + b]; sw += hw[fb + b]; }
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
      if (f == 0 && lane == 0) { tot[0] = P; tot[1] = W; }
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
    if (lane == 0) { f_proxy[f] = bp; f_bin[f] = bb; f_pl[f] = bpl; f_wl[f] = bwl; }
  }
  const int tree = slot_meta[2 * k], node_id = slot_meta[2 * k + 1];
  for (int f = tid; f < n_feat; f += HGBT_BLOCK) f_key[f] = hrf_key(seed, tree, node_id, f);
  __syncthreads();

  for (int f = tid; f < n_feat; f += HGBT_BLOCK) {
    const unsigned long long kf = f_key[f];
    int rank = 0;
    for (int g = 0; g < n_feat; ++g) {  // same g across the wave: LDS broadcast
      const unsigned long long kg = f_key[g];
      rank += (kg < kf || (kg == kf && g < f)) ? 1 : 0;
    }
    f_rank[f] = rank;
    if (f_bin[f] >= 0) atomicMin(&r_star, rank);
  }
  __syncthreads();

  const int limit = max(max_features, r_star + 1);
  HrfPick best;
  best.proxy = 0.0; best.rank = -1; best.feat = -1;
  for (int f = tid; f < n_feat; f += HGBT_BLOCK) {
    if (f_bin[f] < 0 || f_rank[f] >= limit) continue;
    HrfPick c;
    c.proxy = f_proxy[f]; c.rank = f_rank[f]; c.feat = f;
    if (hrf_better(c, best)) best = c;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    HrfPick o;
    o.proxy = __shfl_xor(best.proxy, m);
    o.rank = __shfl_xor(best.rank, m);
    o.feat = __shfl_xor(best.feat, m);
    if (hrf_better(o, best)) best = o;
  }
  if (lane == 0) wave_pick[wave] = best;
  __syncthreads();
  if (tid == 0) {
    for (int wv = 1; wv < HGBT_BLOCK / 64; ++wv)
      if (hrf_better(wave_pick[wv], best)) best = wave_pick[wv];
    long long* o = out + (size_t)k * HRF_REC;
    const bool ok = best.rank >= 0;
    o[0] = __double_as_longlong(ok ? best.proxy : 0.0);
    o[1] = ok ? best.feat : -1;
    o[2] = ok ? f_bin[best.feat] : 0;
    o[3] = ok ? f_pl[best.feat] : 0;
    o[4] = ok ? f_wl[best.feat] : 0;
    o[5] = tot[0]; o[6] = tot[1];
  }
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
// encode_json — parse a /score request body (JSON bytes, the wire format:
// [{"sex": "male", ..., "credit_limit": 18000.0, ...}, ...]) straight into
// (codes, nums) with no intermediate Python objects. This is the serving
// fast path; any deviation from the expected shape throws and the caller
// falls back to the pydantic path for a proper 422. The GIL is released
// during the parse.
// ---------------------------------------------------------------------------

#include <charconv>
#include <cstring>

namespace jsonenc {

struct Error {
  std::string msg;
};

struct Parser {
  const char* p;
  const char* end;

  [[noreturn]] void fail(const char* what) {
    throw Error{std::string(what) + " at offset " + std::to_string((size_t)(p - begin_))};
  }
  const char* begin_;

  void ws() {
    while (p < end && (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r')) ++p;
  }
  bool eat(char c) {
    ws();
    if (p < end && *p == c) { ++p; return true; }
    return false;
  }
  void expect(char c, const char* what) {
    if (!eat(c)) fail(what);
  }

  // Parse a JSON string starting at the opening quote; returns the raw
  // span between quotes and whether it contains escapes. Fast path: one
  // SIMD memchr to the closing quote + one over the span for backslashes
  // (escapes are rare in this schema's values).
  void raw_string(const char*& s, size_t& len, bool& escaped) {
    expect('"', "expected string");
    s = p;
    const char* q = (const char*)std::memchr(p, '"', (size_t)(end - p));
    if (q == nullptr) { p = end; fail("unterminated string"); }
    if (std::memchr(p, '\\', (size_t)(q - p)) == nullptr) {
      escaped = false;
      len = (size_t)(q - s);
      p = q + 1;
      return;
    }
    escaped = true;
    while (p < end) {
      const char c = *p;
      if (c == '"') { len = (size_t)(p - s); ++p; return; }
      if (c == '\\') {
        ++p;
        if (p >= end) break;
      }
      ++p;
    }
    fail("unterminated string");
  }

  // Unescape into buf (capacity cap); returns length or SIZE_MAX if too long.
  size_t unescape(const char* s, size_t len, char* buf, size_t cap) {
    size_t o = 0;
    for (size_t i = 0; i < len; ++i) {
      char c = s[i];
      if (c != '\\') {
        if (o >= cap) return SIZE_MAX;
        buf[o++] = c;
        continue;
      }
      if (++i >= len) return SIZE_MAX;
      c = s[i];
      char repl;
      switch (c) {
        case '"': repl = '"'; break;
        case '\\': repl = '\\'; break;
        case '/': repl = '/'; break;
        case 'b': repl = '\b'; break;
        case 'f': repl = '\f'; break;
        case 'n': repl = '\n'; break;
        case 'r': repl = '\r'; break;
        case 't': repl = '\t'; break;
        case 'u': {
          if (i + 4 >= len) return SIZE_MAX;
          unsigned cp = 0;
          for (int k = 1; k <= 4; ++k) {
            const char h = s[i + k];
            cp <<= 4;
            if (h >= '0' && h <= '9') cp |= (unsigned)(h - '0');
            else if (h >= 'a' && h <= 'f') cp |= (unsigned)(h - 'a' + 10);
            else if (h >= 'A' && h <= 'F') cp |= (unsigned)(h - 'A' + 10);
            else return SIZE_MAX;
          }
          i += 4;
          // UTF-8 encode (surrogate pairs unsupported here: vocab is ASCII,
          // a non-matching value only needs to be *skipped* correctly)
          if (cp < 0x80) {
            if (o >= cap) return SIZE_MAX;
            buf[o++] = (char)cp;
          } else if (cp < 0x800) {
            if (o + 2 > cap) return SIZE_MAX;
            buf[o++] = (char)(0xC0 | (cp >> 6));
            buf[o++] = (char)(0x80 | (cp & 0x3F));
          } else {
            if (o + 3 > cap) return SIZE_MAX;
            buf[o++] = (char)(0xE0 | (cp >> 12));
            buf[o++] = (char)(0x80 | ((cp >> 6) & 0x3F));
            buf[o++] = (char)(0x80 | (cp & 0x3F));
          }
          continue;
        }
        default: return SIZE_MAX;
      }
      if (o >= cap) return SIZE_MAX;
      buf[o++] = repl;
    }
    return o;
  }

  double number() {
    ws();
    double v;
    auto [q, ec] = std::from_chars(p, end, v);
    if (ec != std::errc()) fail("expected number");
    p = q;
    return v;
  }

  bool literal(const char* lit) {
    const size_t n = std::strlen(lit);
    if ((size_t)(end - p) >= n && std::memcmp(p, lit, n) == 0) { p += n; return true; }
    return false;
  }

  void skip_value() {
    ws();
    if (p >= end) fail("truncated value");
    const char c = *p;
    if (c == '"') {
      const char* s; size_t l; bool e;
      raw_string(s, l, e);
    } else if (c == '{' || c == '[') {
      const char open = c, close = (c == '{') ? '}' : ']';
      int depth = 0;
      while (p < end) {
        const char d = *p;
        if (d == '"') { const char* s; size_t l; bool e; raw_string(s, l, e); continue; }
        if (d == open) ++depth;
        else if (d == close && --depth == 0) { ++p; return; }
        ++p;
      }
      fail("unterminated container");
    } else if (literal("null") || literal("true") || literal("false")) {
    } else {
      number();
    }
  }
};

}  // namespace jsonenc

// Persistent encoder state: column dispatch table keyed by
// (key_len << 8) | last_char — one int hash + at most a couple of memcmp
// per field instead of hashing 15-18-char strings 23k times per request.
struct JsonEncoderState {
  std::vector<std::string> key_store;
  std::unordered_map<uint32_t, std::vector<std::pair<int, int>>> dispatch;
  // dispatch value: (key_store index, column id)
  std::vector<std::vector<std::string>> vocab;
  std::vector<int16_t> missing_code;
  std::vector<int16_t> def_codes;
  std::vector<float> def_nums;
  int ncat{}, nnum{};

  JsonEncoderState(py::list vocabs, py::list cat_names, py::list num_names,
                   py::str missing_cat, py::array_t<int16_t> default_codes,
                   py::array_t<float> default_nums) {
    ncat = (int)py::len(cat_names);
    nnum = (int)py::len(num_names);
    vocab.resize(ncat);
    missing_code.assign(ncat, -1);
    const std::string miss = py::cast<std::string>(missing_cat);
    for (int j = 0; j < ncat; ++j) {
      key_store.push_back(py::cast<std::string>(cat_names[j]));
      py::list v = vocabs[j];
      for (ssize_t k = 0; k < py::len(v); ++k) {
        vocab[j].push_back(py::cast<std::string>(v[k]));
        if (vocab[j].back() == miss) missing_code[j] = (int16_t)k;
      }
    }
    for (int j = 0; j < nnum; ++j)
      key_store.push_back(py::cast<std::string>(num_names[j]));
    for (int j = 0; j < ncat + nnum; ++j) {
      const std::string& k = key_store[j];
      const uint32_t h = ((uint32_t)k.size() << 8) | (uint8_t)k.back();
      dispatch[h].emplace_back(j, j);
    }
    TORCH_CHECK((int)default_codes.size() == ncat && (int)default_nums.size() == nnum,
        "default row size mismatch");
    def_codes.assign(default_codes.data(), default_codes.data() + ncat);
    def_nums.assign(default_nums.data(), default_nums.data() + nnum);
  }

  inline int lookup(const char* ks, size_t kl) const {
    if (kl == 0) return -1;
    const uint32_t h = ((uint32_t)kl << 8) | (uint8_t)ks[kl - 1];
    auto it = dispatch.find(h);
    if (it == dispatch.end()) return -1;
    for (const auto& cand : it->second) {
      const std::string& name = key_store[cand.first];
      if (name.size() == kl && std::memcmp(name.data(), ks, kl) == 0)
        return cand.second;
    }
    return -1;
  }
};

// Parse the full body into flat row-major code/num vectors. Caller must
// NOT hold the GIL. Throws jsonenc::Error on malformed input.
static size_t parse_records_nogil(const JsonEncoderState& st, char* data,
                                  ssize_t blen, std::vector<int16_t>& codes,
                                  std::vector<float>& nums) {
  const int ncat = st.ncat;
  const int nnum = st.nnum;
  const auto& vocab = st.vocab;
  const int16_t* def_codes = st.def_codes.data();
  const float* def_nums = st.def_nums.data();
  size_t b = 0;
  {
    jsonenc::Parser P{data, data + blen};
    P.begin_ = data;
    codes.reserve((size_t)blen / 70 * ncat + ncat);
    nums.reserve((size_t)blen / 70 * nnum + nnum);
    {
      P.expect('[', "body must be a JSON array");
      if (!P.eat(']')) {
        do {
          P.expect('{', "record must be an object");
          codes.resize(codes.size() + ncat);
          nums.resize(nums.size() + nnum);
          int16_t* crow = codes.data() + b * ncat;
          float* nrow = nums.data() + b * nnum;
          // absent fields take the schema defaults (pydantic semantics,
          // reference app/model.py:8-34)
          std::memcpy(crow, def_codes, ncat * sizeof(int16_t));
          std::memcpy(nrow, def_nums, nnum * sizeof(float));
          // clients overwhelmingly emit fields in schema order (pydantic
          // model dumps, the sample request, pandas records): try the
          // expected next column with one memcmp before the hash lookup
          int expect_col = 0;
          if (!P.eat('}')) {
            do {
              const char* ks; size_t kl; bool kesc;
              P.raw_string(ks, kl, kesc);
              char kbuf[64];
              if (kesc) {
                const size_t n = P.unescape(ks, kl, kbuf, sizeof(kbuf));
                if (n == SIZE_MAX) P.fail("bad key");
                ks = kbuf; kl = n;
              }
              P.expect(':', "expected ':'");
              int col = -1;
              if (expect_col < ncat + nnum) {
                const std::string& exp = st.key_store[expect_col];
                if (exp.size() == kl && std::memcmp(exp.data(), ks, kl) == 0)
                  col = expect_col;
              }
              if (col < 0) col = st.lookup(ks, kl);
              expect_col = (col >= 0) ? col + 1 : expect_col;
              if (col < 0) {
                P.skip_value();  // extra fields ignored (schema extra="ignore")
              } else if (col < ncat) {
                const int j = col;
                P.ws();
                if (P.p < P.end && *P.p == 'n') {
                  P.fail("null not accepted for a string field");
                } else {
                  const char* vs; size_t vl; bool vesc;
                  P.raw_string(vs, vl, vesc);
                  char vbuf[64];
                  if (vesc) {
                    const size_t n = P.unescape(vs, vl, vbuf, sizeof(vbuf));
                    if (n == SIZE_MAX) { crow[j] = -1; continue; }
                    vs = vbuf; vl = n;
                  }
                  int16_t code = -1;  // unknown category -> all-zero one-hot
                  for (size_t k = 0; k < vocab[j].size(); ++k) {
                    const std::string& cand = vocab[j][k];
                    if (cand.size() == vl && std::memcmp(cand.data(), vs, vl) == 0) {
                      code = (int16_t)k;
                      break;
                    }
                  }
                  crow[j] = code;
                }
              } else {
                const int j = col - ncat;
                P.ws();
                if (P.p < P.end && *P.p == 'n') {
                  P.fail("null not accepted for a numeric field");
                } else {
                  nrow[j] = (float)P.number();
                }
              }
            } while (P.eat(','));
            P.expect('}', "expected '}'");
          }
          ++b;
        } while (P.eat(','));
        P.expect(']', "expected ']'");
      }
      P.ws();
      if (P.p != P.end) P.fail("trailing data");
    }
  }
  return b;
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

// ---------------------------------------------------------------------------
// Drift p-value epilogue on host, in C: chi-square survival via the exact
// closed forms for integer dof (even: Poisson tail sum; odd: erfc +
// half-integer-gamma series, both from the Q(k+2) = Q(k) + term recurrence)
// and the Pelz-Good series for the two-sample K-S p-value (mirrors
// creditcore.models.drift._pelz_good_sf; validated against scipy in
// tests/test_drift_pvals_host.py).
// Replaces ~0.4 ms of numpy/scipy per request with ~5 µs on the Pelz-Good
// path (en >= 300, the serving batch sizes). Small batches cost more: the
// exact matrix (en <= 140, and tiny D below en = 500) and the Smirnov sum
// (140 < en < 300, up to en terms per drifted column) are not timed here.
// ---------------------------------------------------------------------------

static double chi2_sf_int_dof(double x, int dof) {
  if (dof <= 0) return 1.0;
  if (x <= 0.0) return 1.0;
  // Q(1) = erfc(sqrt(x/2)); Q(2) = exp(-x/2);
  // Q(k+2) = Q(k) + (x/2)^(k/2) e^(-x/2) / Gamma(k/2 + 1)
  const double h = 0.5 * x;
  double q, term;
  int k;
  if (dof % 2 == 1) {
    q = std::erfc(std::sqrt(h));
    term = std::sqrt(h / M_PI) * std::exp(-h) * 2.0;  // k=1 increment
    k = 1;
  } else {
    q = std::exp(-h);
    term = h * std::exp(-h);  // k=2 increment
    k = 2;
  }
  while (k + 2 <= dof) {
    q += term;
    k += 2;
    term *= h / (0.5 * k);
  }
  return std::min(1.0, std::max(0.0, q));
}

// Exact P(D_n > d) for small n via the Marsaglia-Tsang-Wang (2003) matrix
// method (Durbin's matrix, one of the exact algorithms scipy's kstwo picks
// from). k-d band is small in practice (k ~ ceil(n d) ~ sqrt(n) near the
// null); the sf underflows to 0 for n d^2 > 18 long before m gets large.
static double mtw_sf(int n, double d) {
  if (d <= 0.0) return 1.0;
  if (d >= 1.0) return 0.0;
  if (n * d * d > 18.0) return 0.0;  // sf < ~2e-16
  const int k = (int)std::ceil(n * d);
  const double h = k - n * d;
  const int m = 2 * k - 1;
  std::vector<double> H((size_t)m * m, 0.0), Q((size_t)m * m, 0.0), tmp((size_t)m * m);
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j)
      if (i - j + 1 >= 0) H[(size_t)i * m + j] = 1.0;
  for (int i = 0; i < m; ++i) {
    H[(size_t)i * m] -= std::pow(h, i + 1);
    H[(size_t)(m - 1) * m + i] -= std::pow(h, m - i);
  }
  H[(size_t)(m - 1) * m] += (2 * h - 1 > 0 ? std::pow(2 * h - 1, m) : 0.0);
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j)
      if (i - j + 1 > 0)
        for (int g = 1; g <= i - j + 1; ++g) H[(size_t)i * m + j] /= g;
  // Q = H^n with power-of-two scaling to avoid under/overflow
  int eH = 0, eQ = 0;
  auto matmul = [&](const std::vector<double>& a, const std::vector<double>& b,
                    std::vector<double>& c) {
    for (int i = 0; i < m; ++i)
      for (int j = 0; j < m; ++j) {
        double s = 0.0;
        for (int g = 0; g < m; ++g) s += a[(size_t)i * m + g] * b[(size_t)g * m + j];
        c[(size_t)i * m + j] = s;
      }
  };
  auto rescale = [&](std::vector<double>& a, int& e) {
    if (a[(size_t)(k - 1) * m + (k - 1)] > 1e140) {
      for (auto& v : a) v *= 1e-140;
      e += 140;
    }
  };
  // initialize Q = I
  for (int i = 0; i < m; ++i) Q[(size_t)i * m + i] = 1.0;
  int nn = n;
  while (nn > 0) {
    if (nn & 1) {
      matmul(Q, H, tmp);
      Q.swap(tmp);
      eQ += eH;
      rescale(Q, eQ);
    }
    matmul(H, H, tmp);
    H.swap(tmp);
    eH *= 2;
    rescale(H, eH);
    nn >>= 1;
  }
  double s = Q[(size_t)(k - 1) * m + (k - 1)];
  // multiply by n! / n^n with the same scaling discipline
  for (int i = 1; i <= n; ++i) {
    s *= (double)i / n;
    if (s < 1e-140) {
      s *= 1e140;
      eQ -= 140;
    }
  }
  const double cdf = s * std::pow(10.0, eQ);
  return std::min(1.0, std::max(0.0, 1.0 - cdf));
}

static double pelz_good_sf(double x, double n) {
  if (x <= 0.0) return 1.0;
  if (x >= 1.0) return 0.0;
  const double z = std::sqrt(n) * x;
  const double z2 = z * z, z3 = z2 * z, z4 = z2 * z2, z6 = z4 * z2;
  const double z7 = z6 * z, z8 = z4 * z4, z10 = z8 * z2;
  const double PI2 = M_PI * M_PI, PI4 = PI2 * PI2, PI6 = PI4 * PI2;
  const double SQRT2PI = std::sqrt(2.0 * M_PI);

  const double qlog = -PI2 / 8.0 / z2;
  if (qlog < -690.0) return 1.0;  // cdf ~ 0
  const double q = std::exp(qlog);

  const double k1a = -z2, k1b = PI2 / 4.0;
  const double k2a = 6 * z6 + 2 * z4;
  const double k2b = (2 * z4 - 5 * z2) * PI2 / 4.0;
  const double k2c = PI4 * (1 - 2 * z2) / 16.0;
  const double k3d = PI6 * (5 - 30 * z2) / 64.0;
  const double k3c = PI4 * (-60 * z2 + 212 * z4) / 16.0;
  const double k3b = PI2 * (135 * z4 - 96 * z6) / 4.0;
  const double k3a = -30 * z6 - 90 * z8;

  double K0 = 0, K1 = 0, K2 = 0, K3 = 0;
  const int maxk = (int)std::ceil(16.0 * z / M_PI);
  for (int k = maxk; k >= 1; --k) {
    const double m = 2.0 * k - 1.0;
    const double m2 = m * m, m4 = m2 * m2, m6 = m4 * m2;
    const double qp = std::pow(q, 8.0 * k);
    K0 = K0 * qp + 1.0;
    K1 = K1 * qp + (k1a + k1b * m2);
    K2 = K2 * qp + (k2a + k2b * m2 + k2c * m4);
    K3 = K3 * qp + (k3a + k3b * m2 + k3c * m4 + k3d * m6);
  }
  K0 *= q * SQRT2PI / z;
  K1 *= q * SQRT2PI / (6 * z4);
  K2 *= q * SQRT2PI / (72 * z7);
  K3 *= q * SQRT2PI / (6480 * z10);

  const double q2 = std::exp(-PI2 / 2.0 / z2);
  double k2x = 0, k3x = 0;
  for (int k = 1; k <= maxk; ++k) {
    const double k2_ = (double)k * k;
    const double qpw = std::pow(q2, k2_);
    k2x += k2_ * qpw;
    const double kspi = M_PI * k;
    const double s3z = std::sqrt(3.0) * z;
    k3x += (s3z + kspi) * (s3z - kspi) * k2_ * qpw;
  }
  K2 += k2x * PI2 * SQRT2PI / (-36 * z3);
  K3 += k3x * PI2 * SQRT2PI / (216 * z6);

  const double sq = std::sqrt(n);
  const double cdf = K0 + K1 / sq + K2 / n + K3 / (n * sq);
  return std::min(1.0, std::max(0.0, 1.0 - cdf));
}

// One-sided Smirnov tail P(D_n^+ >= x), 0 < x < 1, by the Birnbaum-Tingey
// sum x * sum_j C(n,j) (x + j/n)^(j-1) (1 - x - j/n)^(n-j), j <= n(1-x).
// All terms are positive; each is formed in logs, with log C(n,j) carried
// from term to term (three logs and one exp per term, at most n terms).
static double smirnov_sf(int n, double x) {
  const int jmax = (int)std::floor(n * (1.0 - x));
  double sum = 0.0;
  double log_c = 0.0;  // log C(n, j)
  for (int j = 0; j <= jmax; ++j) {
    if (j > 0) log_c += std::log((double)(n - j + 1) / j);
    const double a = x + (double)j / n;
    const double b = 1.0 - x - (double)j / n;
    if (b <= 0.0) continue;  // j = n (1 - x) exactly: the term is 0
    sum += std::exp(log_c + (j - 1) * std::log(a) + (n - j) * std::log(b));
  }
  return std::min(1.0, std::max(0.0, x * sum));
}

static void drift_pvals_raw(const int32_t* bh, const float* kd, int nnum,
                            const int32_t* rc, const int32_t* off, int ncat,
                            int64_t n_ref, int64_t n_batch, double* pv) {

  for (int j = 0; j < ncat; ++j) {
    double rsum = 0, bsum = 0;
    int k = 0;
    const int lo = off[j], hi = off[j + 1];
    for (int i = lo; i < hi; ++i) {
      if (rc[i] + bh[i] > 0) { ++k; rsum += rc[i]; bsum += bh[i]; }
    }
    if (k < 2 || rsum == 0 || bsum == 0) { pv[j] = 1.0; continue; }
    const double n = rsum + bsum;
    double stat = 0;
    for (int i = lo; i < hi; ++i) {
      const double tot = (double)rc[i] + bh[i];
      if (tot <= 0) continue;
      const double er = tot * (rsum / n), eb = tot * (bsum / n);
      double dr = std::fabs(rc[i] - er), db = std::fabs(bh[i] - eb);
      if (k == 2) {  // Yates continuity correction on 2x2
        dr = std::max(dr - 0.5, 0.0);
        db = std::max(db - 0.5, 0.0);
      }
      stat += dr * dr / er + db * db / eb;
    }
    pv[j] = chi2_sf_int_dof(stat, k - 1);
  }

  const double en_f = (double)n_ref * (double)n_batch / ((double)n_ref + (double)n_batch);
  const double en = std::nearbyint(en_f);
  // The target is scipy.stats.kstwo.sf(D, en), what ks_2samp(method="asymp")
  // and so models/drift.ks_asymp_pvalue report. Above n = 140 scipy itself
  // (Simard & L'Ecuyer 2011) selects by region, and so does this:
  //   en <= 140: exact MTW;
  //   en D^2 >= 2.2: twice the one-sided Smirnov tail. Below en = 300 it is
  //     evaluated as such (Pelz-Good is 5e-7 off it at en = 141); from 300
  //     on Pelz-Good stands in, measured <= 1.1e-7 from it;
  //   en D^1.5 <= 1.4: Durbin's exact matrix, i.e. MTW (k <= 1.25 en^(1/3)
  //     + 1, a small matrix). Pelz-Good misses it by 3e-6 at en = 141 and
  //     3.4e-7 at en = 300 but < 3e-7 from en = 320, so this stops at 500;
  //   otherwise Pelz-Good, the same series as scipy's.
  // Checked against kstwo.sf to 3e-7 in tests/test_drift_pvals_host.py.
  for (int j = 0; j < nnum; ++j) {
    const double d = (double)kd[j];
    double p;
    if (en <= 140.0) {
      p = mtw_sf((int)en, d);
    } else if (en < 300.0 && d > 0.0 && d < 1.0 && (en * d) * d >= 2.2) {
      p = std::min(1.0, 2.0 * smirnov_sf((int)en, d));
    } else if (en < 500.0 && en * d * std::sqrt(std::max(d, 0.0)) <= 1.4) {
      p = mtw_sf((int)en, d);
    } else {
      p = pelz_good_sf(d, en);
    }
    pv[ncat + j] = p;
  }
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
  JsonEncoderState st(vocabs, cat_names, num_names, missing_cat,
                      default_codes, default_nums);
  return encode_json_impl(st, body);
}

// ---------------------------------------------------------------------------
// Response serializer: the reference-shaped /score response straight to
// JSON bytes (shortest-round-trip doubles via std::to_chars). Skips the
// Python dict + json.dumps pass on the serving hot path.
// ---------------------------------------------------------------------------

static inline void append_double(std::string& out, double v) {
  char buf[32];
  auto [p, ec] = std::to_chars(buf, buf + sizeof(buf), v);
  (void)ec;
  // JSON requires a fraction or exponent for floats; Python emits "0.0"
  // style. Keep parity: append ".0" to bare integers.
  bool has_dot = false;
  for (char* c = buf; c < p; ++c)
    if (*c == '.' || *c == 'e' || *c == 'E' || *c == 'n' || *c == 'i') { has_dot = true; break; }
  out.append(buf, p);
  if (!has_dot) out += ".0";
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
    out.reserve((size_t)b * 24 + 2048);
    out += "{\"predictions\": [";
    for (int64_t i = 0; i < b; ++i) {
      if (i) out += ", ";
      append_double(out, proba[i]);
    }
    out += "], \"outliers\": [";
    for (int64_t i = 0; i < b; ++i) {
      if (i) out += ", ";
      out += (outlier[i] != 0.0) ? "1.0" : "0.0";
    }
    out += "], \"feature_drift_batch\": {";
    for (int j = 0; j < nf; ++j) {
      if (j) out += ", ";
      out += '\"';
      out += names[j];
      out += "\": ";
      // (1 - p) computed in float32, reference 02-register cell-9 semantics
      append_double(out, (double)(1.0f - (float)pv[j]));
    }
    out += "}}";
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
    out.reserve((size_t)b * 24 + 2048);
    out += "{\"predictions\": [";
    for (int64_t i = 0; i < b; ++i) {
      if (i) out += ", ";
      append_double(out, proba[i]);
    }
    out += "], \"outliers\": [";
    for (int64_t i = 0; i < b; ++i) {
      if (i) out += ", ";
      out += (outl[i] != 0.0) ? "1.0" : "0.0";
    }
    out += "], \"feature_drift_batch\": {";
    for (int j = 0; j < nf; ++j) {
      if (j) out += ", ";
      out += '\"';
      out += names[j];
      out += "\": ";
      append_double(out, (double)(1.0f - (float)pv[j]));
    }
    out += "}}";
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
    out.reserve(b * 24 + 2048);
    out += "{\"predictions\": [";
    for (size_t i = 0; i < b; ++i) {
      if (i) out += ", ";
      append_double(out, proba[i]);
    }
    out += "], \"outliers\": [";
    for (size_t i = 0; i < b; ++i) {
      if (i) out += ", ";
      out += (outlier[i] != 0.0) ? "1.0" : "0.0";
    }
    out += "], \"feature_drift_batch\": {";
    for (int j = 0; j < nf; ++j) {
      if (j) out += ", ";
      out += '\"';
      out += names[j];
      out += "\": ";
      append_double(out, (double)(1.0f - (float)pv[j]));
    }
    out += "}}";
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
    out.reserve((size_t)b * 24 + 2048);
    out += "{\"predictions\": [";
    for (int64_t i = 0; i < b; ++i) {
      if (i) out += ", ";
      append_double(out, proba[i]);
    }
    out += "], \"outliers\": [";
    for (int64_t i = 0; i < b; ++i) {
      if (i) out += ", ";
      out += (outlier[i] != 0.0) ? "1.0" : "0.0";
    }
    out += "], \"feature_drift_batch\": {";
    for (int j = 0; j < nf; ++j) {
      if (j) out += ", ";
      out += '\"';
      out += names[j];
      out += "\": ";
      append_double(out, (double)(1.0f - (float)pv[j]));
    }
    out += "}}";
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
  m.attr("HRF_MAX_ROWS_PER_BLOCK") = py::int_(HRF_MAX_ROWS_PER_BLOCK);
  m.attr("HRF_MAX_FEATS") = py::int_(HRF_MAX_FEATS);
  m.def("drift_stats", &drift_stats,
        "Per-feature drift statistics: categorical histograms + K-S D (gfx950)");
  m.def("encode_records", &encode_records,
        "Native request encoder: list[dict] -> (codes i16[B,9], nums f32[B,14])");
  m.def("encode_json", &encode_json,
        "Parse a /score JSON request body straight into (codes, nums)");
  py::class_<JsonEncoderState>(m, "JsonEncoder")
      .def(py::init<py::list, py::list, py::list, py::str,
                    py::array_t<int16_t>, py::array_t<float>>())
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
