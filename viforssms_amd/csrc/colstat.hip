// Column statistics over a sample-major fp32 matrix x [B][pitch] (include/vissm.h vissm_col_*): per-column
// sum / sum of squares / non-NaN count, and exact per-column order statistics by a 4-pass byte-wise radix select
// on an order-preserving key (colstat_math.hpp).  They replace the reference's host path from posterior samples to
// credible bands (AR.py:323-362 writes every sample with np.savetxt, vis.py takes the quantiles offline) with a
// forward-only summary computed where the samples are.
//
// Layout of every streaming kernel here: a block of 256 threads owns a tile of 32 columns x one slab of rows.  A
// lane keeps one column (tid & 31) and walks the rows tid >> 5, + 8, ..., so a wave reads two 128-byte row
// segments per load with plain dword loads: no alignment beyond the element's 4 bytes is assumed (the product
// passes x[:, 1:] views), and a column's ties land on different LDS words of the same wave only twice.
//
// The select's only cross-block quantity is an integer histogram (LDS ds_add, then one global integer add per
// occupied bin), so its result does not depend on the order of the adds and can be SUM-all-reduced over ranks.
// The moments use no atomics: per-slab double partials in the workspace, then a fixed-order sum over the slabs.
#include "common.hpp"
#include "colstat_math.hpp"

#include <algorithm>

namespace vissm {
namespace {

constexpr int kTC = 32;        // columns per tile
constexpr int kRL = 8;         // row lanes per block (256 threads)
constexpr int kMaxRanks = 16;  // targets per column
constexpr int kHistRowsMax = 4096;  // rows per histogram slab (always below 65536: the LDS counters are 16 bits)
constexpr int kSlotsLate = 3;  // distinct prefixes counted per sweep over the slab in passes 1-3
// words between two LDS histograms: 128 (256 16-bit counters) + 1, so that the same digit of the tile's 32 columns
// falls into 32 different banks (pass 0 of a well-scaled variable: one top byte for nearly every element)
constexpr int kHistPitch = 129;
constexpr int kLoadsAhead = 16;    // row loads a lane of the histogram kernel issues before it uses the first
constexpr int kMomentLoadsAhead = 8;

struct Geo { int n_tiles, rows_per_slab, n_slabs; };

inline int ceil_div(int64_t a, int64_t b) { return static_cast<int>((a + b - 1) / b); }

// rows per slab so that about `want_blocks` blocks exist, between lo and hi rows, a multiple of the 8 row lanes
inline Geo geometry(const VissmColStatDesc& d, int want_blocks, int lo, int64_t hi) {
  Geo g;
  g.n_tiles = ceil_div(d.n_cols, kTC);
  const int slabs_wanted = std::max(1, ceil_div(want_blocks, g.n_tiles));
  int64_t rows = ceil_div(d.B, slabs_wanted);
  rows = std::min<int64_t>(std::max<int64_t>(rows, lo), hi);
  rows = (rows + kRL - 1) / kRL * kRL;
  g.rows_per_slab = static_cast<int>(rows);
  g.n_slabs = ceil_div(d.B, rows);
  return g;
}

// moments: at most 256 slabs (the workspace holds one partial row per slab)
inline Geo moments_geometry(const VissmColStatDesc& d) {
  Geo g = geometry(d, 1024, 64, int64_t{1} << 31);
  if (g.n_slabs > 256) {
    int64_t rows = (ceil_div(d.B, 256) + kRL - 1) / kRL * kRL;
    g.rows_per_slab = static_cast<int>(rows);
    g.n_slabs = ceil_div(d.B, rows);
  }
  return g;
}

// histograms: slabs of at most 4096 rows; beyond 65535 slabs (the grid's y limit) they grow, to 32776 rows at 2^31
inline Geo hist_geometry(const VissmColStatDesc& d) {
  Geo g = geometry(d, 2048, 64, kHistRowsMax);
  if (g.n_slabs > 65535) {
    const int64_t rows = (ceil_div(d.B, 65535) + kRL - 1) / kRL * kRL;
    g.rows_per_slab = static_cast<int>(rows);
    g.n_slabs = ceil_div(d.B, rows);
  }
  return g;
}

int check_desc(const VissmColStatDesc* d, const char* what) {
  VISSM_CHECK_ARG(d, "%s: null descriptor", what);
  VISSM_CHECK_ARG(d->B >= 1 && d->n_cols >= 1 && d->pitch >= d->n_cols,
                  "%s: bad shape (B=%d n_cols=%d pitch=%d)", what, d->B, d->n_cols, d->pitch);
  VISSM_CHECK_ARG(d->n_ranks >= 1 && d->n_ranks <= kMaxRanks, "%s: n_ranks %d outside 1..%d", what, d->n_ranks,
                  kMaxRanks);
  VISSM_CHECK_ARG(static_cast<int64_t>(d->n_cols) * d->n_ranks <= INT32_MAX / 2, "%s: n_cols * n_ranks = %lld too large",
                  what, static_cast<long long>(d->n_cols) * d->n_ranks);
  return VISSM_OK;
}

// ------------------------------------------------------------------------------------------------------------
// moments
// ------------------------------------------------------------------------------------------------------------
// part_s [n_slabs][2][n_cols] double, part_n [n_slabs][n_cols] int32
__global__ __launch_bounds__(256) void col_moments_partial_kernel(VissmColStatDesc d, int rows_per_slab,
                                                                  const float* __restrict__ x,
                                                                  double* __restrict__ part_s,
                                                                  int32_t* __restrict__ part_n) {
  __shared__ double s1[kRL][kTC], s2[kRL][kTC];
  __shared__ int32_t sn[kRL][kTC];
  const int cl = threadIdx.x & (kTC - 1), rl = threadIdx.x >> 5;
  const int c = blockIdx.x * kTC + cl;
  const int64_t r0 = static_cast<int64_t>(blockIdx.y) * rows_per_slab;
  const int64_t r1 = std::min<int64_t>(r0 + rows_per_slab, d.B);
  double a1 = 0.0, a2 = 0.0;
  int32_t n = 0;
  if (c < d.n_cols) {
    const float* p = x + c;
    auto add = [&](float v) {
      if (v == v) {
        const double dv = static_cast<double>(v);
        a1 += dv;
        a2 += dv * dv;
        ++n;
      }
    };
    // rows in ascending order whatever the batching: the sum's order is fixed
    const int64_t step = static_cast<int64_t>(kRL) * d.pitch;
    int64_t r = r0 + rl;
    const float* q = p + r * d.pitch;
    for (; r + (kMomentLoadsAhead - 1) * kRL < r1; r += kMomentLoadsAhead * kRL, q += kMomentLoadsAhead * step) {
      float v[kMomentLoadsAhead];
#pragma unroll
      for (int j = 0; j < kMomentLoadsAhead; ++j) v[j] = q[j * step];
#pragma unroll
      for (int j = 0; j < kMomentLoadsAhead; ++j) add(v[j]);
    }
    for (; r < r1; r += kRL, q += step) add(*q);
  }
  s1[rl][cl] = a1;
  s2[rl][cl] = a2;
  sn[rl][cl] = n;
  __syncthreads();
  if (rl == 0 && c < d.n_cols) {
    for (int i = 1; i < kRL; ++i) {  // fixed order
      a1 += s1[i][cl];
      a2 += s2[i][cl];
      n += sn[i][cl];
    }
    const int64_t slab = blockIdx.y;
    part_s[(slab * 2 + 0) * d.n_cols + c] = a1;
    part_s[(slab * 2 + 1) * d.n_cols + c] = a2;
    part_n[slab * d.n_cols + c] = n;
  }
}

__global__ __launch_bounds__(256) void col_moments_reduce_kernel(int n_cols, int n_slabs,
                                                                 const double* __restrict__ part_s,
                                                                 const int32_t* __restrict__ part_n,
                                                                 double* __restrict__ sums,
                                                                 int32_t* __restrict__ n_valid) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_cols) return;
  double a1 = 0.0, a2 = 0.0;
  int32_t n = 0;
  for (int64_t s = 0; s < n_slabs; ++s) {  // fixed order
    a1 += part_s[(s * 2 + 0) * n_cols + c];
    a2 += part_s[(s * 2 + 1) * n_cols + c];
    n += part_n[s * n_cols + c];
  }
  sums[c] = a1;
  sums[n_cols + c] = a2;
  n_valid[c] = n;
}

// ------------------------------------------------------------------------------------------------------------
// radix select: one byte's histograms
// ------------------------------------------------------------------------------------------------------------
// Targets of a column whose keys agree above the current byte (all of them in pass 0) share one LDS histogram, a
// "slot"; SLOTS of them are counted per sweep over the slab and the sweep repeats until every distinct prefix of
// the tile's columns has been counted.  LDS counters are 16 bits, two to a word: a slab has fewer than 65536 rows.
template <int SLOTS>
__global__ __launch_bounds__(256) void col_hist_kernel(VissmColStatDesc d, int rows_per_slab, int pass,
                                                       const float* __restrict__ x,
                                                       const uint32_t* __restrict__ prefix,
                                                       int32_t* __restrict__ hist) {
  __shared__ uint32_t cnt[kTC * SLOTS * kHistPitch];
  __shared__ uint32_t s_above[kTC][kMaxRanks];  // distinct key parts above this byte, per column
  __shared__ uint8_t s_slot[kTC][kMaxRanks];    // target -> index into s_above
  __shared__ int s_nd[kTC];
  __shared__ int s_max_nd;
  const int tid = threadIdx.x;
  const int cl = tid & (kTC - 1), rl = tid >> 5;
  const int c0 = blockIdx.x * kTC;
  const int c = c0 + cl;
  const int nr = d.n_ranks;
  const int shift = cs::pass_shift(pass);
  const int64_t r0 = static_cast<int64_t>(blockIdx.y) * rows_per_slab;
  const int64_t r1 = std::min<int64_t>(r0 + rows_per_slab, d.B);

  if (tid == 0) s_max_nd = 0;
  __syncthreads();
  if (tid < kTC) {
    int nd = 0;
    if (c0 + tid < d.n_cols) {
      for (int r = 0; r < nr; ++r) {
        const uint32_t a = cs::key_above(prefix[static_cast<int64_t>(c0 + tid) * nr + r], pass);
        int j = 0;
        while (j < nd && s_above[tid][j] != a) ++j;
        if (j == nd) s_above[tid][nd++] = a;
        s_slot[tid][r] = static_cast<uint8_t>(j);
      }
    }
    s_nd[tid] = nd;
    atomicMax(&s_max_nd, nd);
  }
  __syncthreads();
  const int max_nd = s_max_nd;
  const int my_nd = s_nd[cl];

  for (int g0 = 0; g0 < max_nd; g0 += SLOTS) {
    for (int i = tid; i < kTC * SLOTS * kHistPitch; i += 256) cnt[i] = 0u;
    uint32_t want[SLOTS];
    bool live[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      live[s] = g0 + s < my_nd;
      want[s] = live[s] ? s_above[cl][g0 + s] : 0u;
    }
    __syncthreads();
    if (c < d.n_cols && live[0]) {
      const float* p = x + c;
      auto count = [&](float v) {
        const uint32_t key = cs::colkey(v);
        const uint32_t above = cs::key_above(key, pass);
        const uint32_t digit = (key >> shift) & 255u;
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
          if (live[s] && above == want[s])
            atomicAdd(&cnt[(cl * SLOTS + s) * kHistPitch + (digit >> 1)], 1u << ((digit & 1u) * 16));
        }
      };
      // kLoadsAhead independent row loads per lane before the first is used: the bytes in flight, not the
      // arithmetic, set this kernel's rate (profiles/r11/summary)
      const int64_t step = static_cast<int64_t>(kRL) * d.pitch;
      int64_t r = r0 + rl;
      const float* q = p + r * d.pitch;
      for (; r + (kLoadsAhead - 1) * kRL < r1; r += kLoadsAhead * kRL, q += kLoadsAhead * step) {
        float v[kLoadsAhead];
#pragma unroll
        for (int j = 0; j < kLoadsAhead; ++j) v[j] = q[j * step];
#pragma unroll
        for (int j = 0; j < kLoadsAhead; ++j) count(v[j]);
      }
      for (; r < r1; r += kRL, q += step) count(*q);
    }
    __syncthreads();
    // one global integer add per occupied bin and target of the slot
    for (int i = tid; i < kTC * SLOTS * kHistPitch; i += 256) {
      const uint32_t w = cnt[i];
      if (w == 0u) continue;  // (the pad word stays 0)
      const int col = i / (SLOTS * kHistPitch), s = (i / kHistPitch) % SLOTS, word = i % kHistPitch;
      const int slot = g0 + s;
      for (int r = 0; r < nr; ++r) {
        if (s_slot[col][r] != slot) continue;
        int32_t* h = hist + (static_cast<int64_t>(c0 + col) * nr + r) * 256 + 2 * word;
        if (w & 0xFFFFu) atomicAdd(h, static_cast<int32_t>(w & 0xFFFFu));
        if (w >> 16) atomicAdd(h + 1, static_cast<int32_t>(w >> 16));
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void col_narrow_kernel(int n, int pass, const int32_t* __restrict__ hist,
                                                         int32_t* __restrict__ rank_left,
                                                         uint32_t* __restrict__ prefix) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int32_t r = rank_left[i];
  uint32_t p = prefix[i];
  if (pass == 0) p = 0u;
  cs::col_narrow(hist + static_cast<int64_t>(i) * 256, &r, &p, pass);
  rank_left[i] = r;
  prefix[i] = p;
}

__global__ __launch_bounds__(256) void col_decode_kernel(int n_cols, int n_ranks, const uint32_t* __restrict__ prefix,
                                                         float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;  // over [n_ranks][n_cols], columns fastest
  if (i >= n_cols * n_ranks) return;
  const int r = i / n_cols, c = i % n_cols;
  out[i] = cs::colkey_inv(prefix[static_cast<int64_t>(c) * n_ranks + r]);
}

}  // namespace
}  // namespace vissm

using namespace vissm;

extern "C" size_t vissm_col_moments_workspace_size(const VissmColStatDesc* d) {
  if (check_desc(d, "col_moments") != VISSM_OK) return 0;
  const Geo g = moments_geometry(*d);
  return align_up(static_cast<size_t>(g.n_slabs) * 2 * d->n_cols * sizeof(double)) +
         align_up(static_cast<size_t>(g.n_slabs) * d->n_cols * sizeof(int32_t));
}

extern "C" int vissm_col_moments(const VissmColStatDesc* d, const float* x, double* sums, int32_t* n_valid,
                                 void* workspace, void* stream) {
  if (int rc = check_desc(d, "col_moments")) return rc;
  VISSM_CHECK_ARG(x && sums && n_valid && workspace, "col_moments: null pointer");
  const Geo g = moments_geometry(*d);
  double* part_s = static_cast<double*>(workspace);
  int32_t* part_n = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) +
                                               align_up(static_cast<size_t>(g.n_slabs) * 2 * d->n_cols * sizeof(double)));
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(col_moments_partial_kernel, dim3(g.n_tiles, g.n_slabs), dim3(256), 0, st, *d, g.rows_per_slab, x,
                     part_s, part_n);
  VISSM_CHECK_LAUNCH("col_moments (partials)");
  hipLaunchKernelGGL(col_moments_reduce_kernel, dim3((d->n_cols + 255) / 256), dim3(256), 0, st, d->n_cols, g.n_slabs,
                     part_s, part_n, sums, n_valid);
  VISSM_CHECK_LAUNCH("col_moments (reduce)");
  return VISSM_OK;
}

// The histograms are summed straight into the caller's `hist`; the workspace is reserved (one aligned unit) so the
// call keeps the ABI's shape should a slab reducer replace the integer adds.
extern "C" size_t vissm_col_select_workspace_size(const VissmColStatDesc* d) {
  if (check_desc(d, "col_select") != VISSM_OK) return 0;
  return align_up(1);
}

extern "C" int vissm_col_select_hist(const VissmColStatDesc* d, const float* x, const uint32_t* prefix, int32_t pass,
                                     int32_t* hist, void* workspace, void* stream) {
  if (int rc = check_desc(d, "col_select_hist")) return rc;
  VISSM_CHECK_ARG(x && prefix && hist, "col_select_hist: null pointer");
  VISSM_CHECK_ARG(pass >= 0 && pass <= 3, "col_select_hist: pass %d outside 0..3", pass);
  (void)workspace;
  const Geo g = hist_geometry(*d);
  VISSM_CHECK_ARG(g.n_slabs <= 65535 && g.rows_per_slab < 65536, "col_select_hist: B=%d needs %d row slabs", d->B,
                  g.n_slabs);
  hipStream_t st = as_stream(stream);
  const size_t bytes = static_cast<size_t>(d->n_cols) * d->n_ranks * 256 * sizeof(int32_t);
  if (hipMemsetAsync(hist, 0, bytes, st) != hipSuccess) {
    set_error("col_select_hist: clearing the histograms failed");
    return VISSM_ELAUNCH;
  }
  if (pass == 0)
    hipLaunchKernelGGL(col_hist_kernel<1>, dim3(g.n_tiles, g.n_slabs), dim3(256), 0, st, *d, g.rows_per_slab, pass, x,
                       prefix, hist);
  else
    hipLaunchKernelGGL(col_hist_kernel<kSlotsLate>, dim3(g.n_tiles, g.n_slabs), dim3(256), 0, st, *d, g.rows_per_slab,
                       pass, x, prefix, hist);
  VISSM_CHECK_LAUNCH("col_select_hist");
  return VISSM_OK;
}

extern "C" int vissm_col_select_narrow(const VissmColStatDesc* d, const int32_t* hist, int32_t* rank_left,
                                       uint32_t* prefix, int32_t pass, void* stream) {
  if (int rc = check_desc(d, "col_select_narrow")) return rc;
  VISSM_CHECK_ARG(hist && rank_left && prefix, "col_select_narrow: null pointer");
  VISSM_CHECK_ARG(pass >= 0 && pass <= 3, "col_select_narrow: pass %d outside 0..3", pass);
  const int n = d->n_cols * d->n_ranks;
  hipLaunchKernelGGL(col_narrow_kernel, dim3((n + 255) / 256), dim3(256), 0, as_stream(stream), n, pass, hist,
                     rank_left, prefix);
  VISSM_CHECK_LAUNCH("col_select_narrow");
  return VISSM_OK;
}

extern "C" int vissm_col_select_decode(const VissmColStatDesc* d, const uint32_t* prefix, float* out, void* stream) {
  if (int rc = check_desc(d, "col_select_decode")) return rc;
  VISSM_CHECK_ARG(prefix && out, "col_select_decode: null pointer");
  const int n = d->n_cols * d->n_ranks;
  hipLaunchKernelGGL(col_decode_kernel, dim3((n + 255) / 256), dim3(256), 0, as_stream(stream), d->n_cols, d->n_ranks,
                     prefix, out);
  VISSM_CHECK_LAUNCH("col_select_decode");
  return VISSM_OK;
}
