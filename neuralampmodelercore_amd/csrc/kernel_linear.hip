// kernel_linear.hip — Linear models (nam::Linear, NAM/linear.cpp:168-196): y[n] = bias + sum_{k < R} h[k] x[n - k], one impulse
// response for every column (column = stream x channels-per-stream + channel). plan.h: LinearPlan, kernels.h: LinearArgs.
//
// A launch piece (n_frames <= the batch's piece length) is three kernels on one stream:
//   nam_linear_append_kernel   planar input [stream][ch][frame] -> hist[(pos + frame) mod L][column]   (transposed through LDS:
//                              reads coalesced along frames, writes along columns)
//   nam_linear_kernel          grid = column tiles (32) x K-splits x frame tiles (64), one wavefront each:
//                              part[split][frame][column] = sum over the split's taps, on v_mfma_f32_32x32x2_f32 — exact f32, a k-ordered
//                              fmaf chain. The K index of the GEMM is the history frame q: B row q = hist row (pos + q) mod L, one coalesced
//                              128-byte read per 32 lanes; A[frame][q] = h[frame - q], the Toeplitz matrix of the IR, never materialised:
//                              lane (i, k) reads ONE float of the split's taps from LDS, where they sit between two zero pads of 64 —
//                              the triangles at both ends of the split (lags outside [t0, t0 + split_taps)) multiply zeros.
//   nam_linear_reduce_kernel   out[stream][ch][frame] = bias + part[0] + part[1] + ... in split order (no atomics: the same bits
//                              every run, at every stream count), transposed back through LDS
//   (+ nam_linear_zero_kernel  output channels >= min(in, out) are 0, not the bias: linear.cpp:191-195)
// Padded columns (n_cols .. cols_pad) of hist are never written and stay zero; they are computed on zeros and not stored to `out`.
// A last partial frame tile computes all 64 frames (on older ring rows: finite, and a frame never sees a later row) and stores
// only its own.
//
// A SlimmableContainer whose submodels are all Linear (kernels.h: LinearPairsArgs, linear_worklist.h) keeps the same ring for streams
// that run different impulse responses, and a piece is again three kernels: the append kernel as above, nam_linear_pairs_kernel over a
// work list of (column tile, submodel) pairs — the wavefront's work is the SAME function, linear_tile, with the pair's taps and
// splits — and nam_linear_pairs_reduce_kernel, where every column sums its own pair's splits and adds its own submodel's bias.
#include "kernels.h"

namespace namhip
{
namespace
{
constexpr int kTileF = kBlock, kTileC = kLinearColTile, kLdsPitch = kTileF + 1; // [column][frame] tile, odd pitch: no bank conflicts either way

__global__ __launch_bounds__(256) void nam_linear_append_kernel(const LinearArgs a)
{
  __shared__ float tile[kTileC * kLdsPitch];
  const int col0 = blockIdx.x * kTileC, f0 = blockIdx.y * kTileF, tid = threadIdx.x;
  {
    const int f = tid & 63, cg = tid >> 6;
    for (int j = 0; j < 8; j++)
    {
      const int c = cg * 8 + j, col = col0 + c;
      float v = 0.0f;
      if (a.in && col < a.n_cols && f0 + f < a.n_frames)
      {
        const int s = col / a.cols_per_stream, ch = col - s * a.cols_per_stream;
        v = a.in[((size_t)s * a.in_ch + ch) * a.io_stride + f0 + f];
      }
      tile[c * kLdsPitch + f] = v;
    }
  }
  __syncthreads();
  {
    const int c = tid & 31, fr = tid >> 5;
    if (col0 + c >= a.n_cols)
      return;
    for (int j = 0; j < 8; j++)
    {
      const int f = fr * 8 + j;
      if (f0 + f >= a.n_frames)
        break;
      int row = a.pos + f0 + f; // (pos < L and a piece is shorter than L: one wrap at most)
      if (row >= a.hist_frames)
        row -= a.hist_frames;
      a.hist[(size_t)row * a.cols_pad + col0 + c] = tile[c * kLdsPitch + f];
    }
  }
}

__global__ __launch_bounds__(256) void nam_linear_reduce_kernel(const LinearArgs a)
{
  __shared__ float tile[kTileC * kLdsPitch];
  const int col0 = blockIdx.x * kTileC, f0 = blockIdx.y * kTileF, tid = threadIdx.x;
  {
    const int c = tid & 31, fr = tid >> 5;
    for (int j = 0; j < 8; j++)
    {
      const int f = fr * 8 + j; // (f0 + f < part_frames: every row of the tile exists in `part`)
      const float* p = a.part + (size_t)(f0 + f) * a.cols_pad + col0 + c;
      const size_t split_pitch = (size_t)a.part_frames * a.cols_pad;
      float acc = 0.0f;
      int s = 0;
      for (; s + 8 <= a.n_splits; s += 8) // fixed order; eight requests in flight (a thread's 8 x n_splits reads are otherwise one round trip each)
      {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; u++)
          v[u] = p[(size_t)(s + u) * split_pitch];
#pragma unroll
        for (int u = 0; u < 8; u++)
          acc += v[u];
      }
      for (; s < a.n_splits; s++)
        acc += p[(size_t)s * split_pitch];
      tile[c * kLdsPitch + f] = acc + a.bias; // the bias last (linear.cpp:186)
    }
  }
  __syncthreads();
  {
    const int f = tid & 63, cg = tid >> 6;
    if (f0 + f >= a.n_frames)
      return;
    for (int j = 0; j < 8; j++)
    {
      const int c = cg * 8 + j, col = col0 + c;
      if (col >= a.n_cols)
        break;
      const int s = col / a.cols_per_stream, ch = col - s * a.cols_per_stream;
      a.out[((size_t)s * a.out_ch + ch) * a.io_stride + f0 + f] = tile[c * kLdsPitch + f];
    }
  }
}

// rows (stream, ch >= cols_per_stream) of `out`, frames [0, n_frames)
__global__ __launch_bounds__(256) void nam_linear_zero_kernel(const LinearArgs a)
{
  const int extra = a.out_ch - a.cols_per_stream;
  const int row = blockIdx.x, s = row / extra, ch = a.cols_per_stream + row - s * extra;
  const int f = blockIdx.y * 256 + threadIdx.x;
  if (f < a.n_frames)
    a.out[((size_t)s * a.out_ch + ch) * a.io_stride + f] = 0.0f;
}
} // namespace

typedef float lin_f16 __attribute__((ext_vector_type(16)));

// One wavefront's work, shared by nam_linear_kernel (one impulse response for the batch) and nam_linear_pairs_kernel (one per work-list
// pair): the 64 output frames from F0 of the 32 columns from col0, over the taps [t0, t0 + KS) of the impulse response whose lag 0
// is a.blob[taps_off]. The partial sums go to pp[frame * part_pitch + lane's column] (pp: frame F0 of the split's slab, column 0 of the tile).
// Inlined into both: the one-model kernel keeps its instructions (profiles/linear_container/README.md compares the listings).
__device__ __forceinline__ void linear_tile(const LinearArgs& a, const int taps_off, const int KS, const int t0, const int col0, const int F0,
                                            float* pp_tile, const int part_pitch)
{
  extern __shared__ float hs[]; // [64 zeros | the split's taps | 64 zeros]: hs[j] = h[t0 + j - 64]
  const int lane = threadIdx.x;
  const int L = a.hist_frames;
  for (int j = lane; j < KS + 2 * kLinearPad; j += 64)
  {
    const int t = j - kLinearPad;
    hs[j] = (t >= 0 && t < KS) ? a.blob[taps_off + t0 + t] : 0.0f; // (taps behind R are zeros in the blob)
  }
  __syncthreads();
  const int i = lane & 31, kk = lane >> 5;
  // step s feeds history frames q = F0 - t0 - KS + 2 s + kk (relative to the piece's frame 0), oldest first; output frame
  // F0 + 32 m + i takes it at lag F0 + 32 m + i - q, i.e. hs[32 m + i + KS + 64 - 2 s - kk]: from KS + 127 down to 1
  int row = a.pos + F0 - t0 - KS + kk; // in (-L, 2 L): hist_frames >= n_splits * KS + the piece, the piece >= F0 + 64
  if (row < 0)
    row += L;
  if (row >= L)
    row -= L;
  const float* hp = a.hist + col0 + i;
  int ja = i + KS + kLinearPad - kk;
  lin_f16 acc0, acc1;
  for (int v = 0; v < 16; v++)
    acc0[v] = acc1[v] = 0.0f;
  // groups of eight steps, the next group's history rows requested before the current group's sixteen matrix instructions
  // (1,024 cycles: a memory round trip) are issued. (KS + 64) / 2 steps: a multiple of 32, so the group count is even.
  auto load8 = [&](float (&b)[8]) {
#pragma unroll
    for (int u = 0; u < 8; u++)
    {
      int rr = row + 2 * u; // (row < L and L >= 16: one wrap at most)
      if (rr >= L)
        rr -= L;
      b[u] = hp[(size_t)rr * a.cols_pad];
    }
    row += 16;
    if (row >= L)
      row -= L;
  };
  auto mma8 = [&](const float (&b)[8]) {
#pragma unroll
    for (int u = 0; u < 8; u++)
    {
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(hs[ja - 2 * u], b[u], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(hs[ja - 2 * u + 32], b[u], acc1, 0, 0, 0);
    }
    ja -= 16;
  };
  const int groups = (KS + kBlock) / 16;
  float b0[8], b1[8];
  load8(b0);
  for (int g = 0; g < groups; g += 2)
  {
    // (the scheduler otherwise sinks a group's requests below the matrix instructions in front of them: a round trip exposed per pair)
    load8(b1);
    __builtin_amdgcn_sched_barrier(0);
    mma8(b0);
    __builtin_amdgcn_sched_barrier(0);
    if (g + 2 < groups)
      load8(b0);
    __builtin_amdgcn_sched_barrier(0);
    mma8(b1);
  }
  // D: lane holds column i, rows (v & 3) + 8 (v >> 2) + 4 kk. Every row of the tile exists in `part` (part_frames is a multiple of 64).
  float* pp = pp_tile + i;
  for (int v = 0; v < 16; v++)
  {
    const int r = (v & 3) + 8 * (v >> 2) + 4 * kk;
    pp[(size_t)r * part_pitch] = acc0[v];
    pp[(size_t)(r + 32) * part_pitch] = acc1[v];
  }
}

__global__ __launch_bounds__(64) void nam_linear_kernel(const LinearArgs a)
{
  const int col0 = blockIdx.x * kLinearColTile, split = blockIdx.y, F0 = blockIdx.z * kBlock;
  linear_tile(a, a.taps_off, a.split_taps, split * a.split_taps, col0, F0,
              a.part + ((size_t)split * a.part_frames + F0) * a.cols_pad + col0, a.cols_pad);
}

// The container form (kernels.h: LinearPairsArgs): workgroup (x, y, z) = (work-list pair, K-split, frame tile). The pair names its
// column tile and its submodel's taps and splits; a pair with fewer splits than the grid's extent leaves at once. Partial sums to
// part[pair's slab + split][frame][32].
__global__ __launch_bounds__(64) void nam_linear_pairs_kernel(const LinearPairsArgs p)
{
  const LinearPair e = p.pairs[blockIdx.x];
  const int split = blockIdx.y, F0 = blockIdx.z * kBlock;
  if (split >= e.n_splits)
    return;
  linear_tile(p.a, e.taps_off, e.split_taps, split * e.split_taps, e.col_tile * kLinearColTile, F0,
              p.a.part + ((size_t)(e.part_slab + split) * p.a.part_frames + F0) * kLinearColTile, kLinearColTile);
}

namespace
{
// out[stream][frame] = its pair's part[slab + 0] + part[slab + 1] + ... in split order + its submodel's bias, transposed back through
// LDS as nam_linear_reduce_kernel does (column = stream: the container is 1-in / 1-out)
__global__ __launch_bounds__(256) void nam_linear_pairs_reduce_kernel(const LinearPairsArgs p)
{
  __shared__ float tile[kTileC * kLdsPitch];
  const LinearArgs& a = p.a;
  const int col0 = blockIdx.x * kTileC, f0 = blockIdx.y * kTileF, tid = threadIdx.x;
  {
    const int c = tid & 31, fr = tid >> 5;
    const int pair = p.col_pair[col0 + c]; // (-1: padding behind the last stream, never stored)
    LinearPair e;
    e.n_splits = 0, e.part_slab = 0, e.bias = 0.0f;
    if (pair >= 0)
      e = p.pairs[pair];
    const size_t split_pitch = (size_t)a.part_frames * kLinearColTile;
    for (int j = 0; j < 8; j++)
    {
      const int f = fr * 8 + j; // (f0 + f < part_frames: every row of the tile exists in `part`)
      const float* q = a.part + (size_t)e.part_slab * split_pitch + (size_t)(f0 + f) * kLinearColTile + c;
      float acc = 0.0f;
      int s = 0;
      for (; s + 8 <= e.n_splits; s += 8) // the order and the grouping of nam_linear_reduce_kernel
      {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; u++)
          v[u] = q[(size_t)(s + u) * split_pitch];
#pragma unroll
        for (int u = 0; u < 8; u++)
          acc += v[u];
      }
      for (; s < e.n_splits; s++)
        acc += q[(size_t)s * split_pitch];
      tile[c * kLdsPitch + f] = acc + e.bias; // the bias last (linear.cpp:186)
    }
  }
  __syncthreads();
  {
    const int f = tid & 63, cg = tid >> 6;
    if (f0 + f >= a.n_frames)
      return;
    for (int j = 0; j < 8; j++)
    {
      const int col = col0 + cg * 8 + j;
      if (col >= a.n_cols)
        break;
      a.out[(size_t)col * a.io_stride + f0 + f] = tile[(cg * 8 + j) * kLdsPitch + f];
    }
  }
}
} // namespace

hipError_t launch_linear(const LinearArgs& a, hipStream_t stream)
{
  // the geometry the kernels' index arithmetic relies on (tools/src/linear_index_check.cpp walks the same arithmetic on the host)
  if (a.n_frames <= 0 || a.n_frames > a.part_frames || a.part_frames % kBlock != 0 || a.part_frames > kLinearPieceMax || a.cols_pad % kLinearColTile != 0 || a.n_cols > a.cols_pad
      || a.n_cols != a.n_streams * a.cols_per_stream || a.split_taps % kBlock != 0 || a.n_splits < 1
      || a.hist_frames < a.n_splits * a.split_taps + a.part_frames - (kBlock - 1) || a.pos < 0 || a.pos >= a.hist_frames
      || a.io_stride < a.n_frames || a.cols_per_stream < 1 || a.cols_per_stream > a.in_ch || a.cols_per_stream > a.out_ch)
    return hipErrorInvalidValue;
  const dim3 tiles(a.cols_pad / kLinearColTile, (a.n_frames + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(nam_linear_append_kernel, tiles, dim3(256), 0, stream, a);
  if (a.out)
  {
    const int lds = (a.split_taps + 2 * kLinearPad) * (int)sizeof(float);
    hipLaunchKernelGGL(nam_linear_kernel, dim3(tiles.x, a.n_splits, tiles.y), dim3(64), lds, stream, a);
    hipLaunchKernelGGL(nam_linear_reduce_kernel, tiles, dim3(256), 0, stream, a);
    if (a.out_ch > a.cols_per_stream)
      hipLaunchKernelGGL(nam_linear_zero_kernel, dim3(a.n_streams * (a.out_ch - a.cols_per_stream), (a.n_frames + 255) / 256), dim3(256), 0,
                         stream, a);
  }
  return hipGetLastError();
}

hipError_t launch_linear_pairs(const LinearPairsArgs& p, hipStream_t stream)
{
  // launch_linear's geometry with one column per stream; a.n_splits and a.split_taps bound every pair's (the host checks the table
  // it uploads: api_launch.cpp, lin_container_upload)
  const LinearArgs& a = p.a;
  if (a.n_frames <= 0 || a.n_frames > a.part_frames || a.part_frames % kBlock != 0 || a.part_frames > kLinearPieceMax || a.cols_pad % kLinearColTile != 0
      || a.n_cols > a.cols_pad || a.n_cols != a.n_streams || a.cols_per_stream != 1 || a.in_ch != 1 || a.out_ch != 1 || a.split_taps % kBlock != 0
      || a.n_splits < 1 || p.hist_taps < a.split_taps || a.hist_frames < p.hist_taps + a.part_frames - (kBlock - 1) || a.pos < 0
      || a.pos >= a.hist_frames || a.io_stride < a.n_frames || p.n_pairs < a.cols_pad / kLinearColTile || !p.pairs || !p.col_pair)
    return hipErrorInvalidValue;
  const dim3 tiles(a.cols_pad / kLinearColTile, (a.n_frames + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(nam_linear_append_kernel, tiles, dim3(256), 0, stream, a);
  if (a.out)
  {
    const int lds = (a.split_taps + 2 * kLinearPad) * (int)sizeof(float);
    hipLaunchKernelGGL(nam_linear_pairs_kernel, dim3(p.n_pairs, a.n_splits, tiles.y), dim3(64), lds, stream, p);
    hipLaunchKernelGGL(nam_linear_pairs_reduce_kernel, tiles, dim3(256), 0, stream, p);
  }
  return hipGetLastError();
}

} // namespace namhip
