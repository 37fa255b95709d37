// kernel_a2_transcode.hip — nam_a2_transcode_kernel: a narrow A2 container submodel's streams between nam_wn_reg_kernel's state and
// the zero-padded rings of the largest submodel's layout (a2_transcode.h: the table, and why ring row i of one side is ring row i
// of the other). One workgroup per (ring, stream); a thread moves one float of the padded side at a time, channels fastest, so the
// padded rows are whole 32-byte accesses and the narrow side is read / written in its groups of up to four channels. It moves
// data and does no arithmetic: to the padded side the channels the narrow model does not have become +0, the other way they are
// dropped; the ring's write position goes along. Runs inside control calls only (api_launch.cpp: mix_enter / mix_leave, the
// stream slots), on the batch's stream, with the batch quiesced.
// Behind it nam_state_rows_copy_kernel, the mover of a residency whose two sides keep ONE layout (the official WaveNet topology's
// lite and feather submodels next to the standard one: api_internal.h, MIX_A1): whole state rows, bit for bit.
#include <algorithm>

#include "device_common.h"
#include "kernels.h"

namespace namhip
{
__global__ __launch_bounds__(256) void nam_a2_transcode_kernel(const A2XcRing* __restrict__ rings, float* __restrict__ a2_state, long a2_stride,
                                                               float* __restrict__ wr_state, long wr_stride, const int* __restrict__ streams,
                                                               int to_padded)
{
  __shared__ A2XcRing r;
  {
    static_assert(sizeof(A2XcRing) % 4 == 0 && sizeof(A2XcRing) / 4 <= 256, "one word per thread");
    const int* src = reinterpret_cast<const int*>(rings + blockIdx.x);
    if (threadIdx.x < sizeof(A2XcRing) / 4)
      reinterpret_cast<int*>(&r)[threadIdx.x] = src[threadIdx.x];
  }
  __syncthreads();
  const int stream = streams ? streams[blockIdx.y] : (int)blockIdx.y;
  float* const A = a2_state + (size_t)stream * (size_t)a2_stride;
  float* const W = wr_state + (size_t)stream * (size_t)wr_stride;
  const int n = r.R * r.a2_ch;
  for (int e = (int)threadIdx.x; e < n; e += 256)
  {
    const int i = e / r.a2_ch, c = e - i * r.a2_ch;
    if (to_padded)
      A[r.a2_off + e] = c < r.wr_ch ? W[r.wr_off[c] + i * r.wr_gs[c]] : 0.0f;
    else if (c < r.wr_ch)
      W[r.wr_off[c] + i * r.wr_gs[c]] = A[r.a2_off + e];
  }
  if (threadIdx.x == 0)
  {
    int* const ap = reinterpret_cast<int*>(A) + r.ring_id;
    int* const wp = reinterpret_cast<int*>(W) + r.slot;
    if (to_padded)
      *ap = *wp;
    else
      *wp = *ap;
  }
}

// `rings`: the device copy of a table that passed a2_transcode_check against rows of at least its two state sizes; `streams`:
// n_streams stream indices in device memory (nullptr: streams 0 .. n_streams - 1)
hipError_t launch_a2_transcode(const A2XcRing* rings, int n_rings, float* a2_state, long a2_stride, float* wr_state, long wr_stride,
                               const int* streams, int n_streams, bool to_padded, hipStream_t stream)
{
  if (n_rings <= 0 || n_streams <= 0)
    return hipSuccess;
  if (!rings || !a2_state || !wr_state || n_streams > 65535)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(nam_a2_transcode_kernel, dim3((unsigned)n_rings, (unsigned)n_streams), dim3(256), 0, stream, rings, a2_state, a2_stride,
                     wr_state, wr_stride, streams, to_padded ? 1 : 0);
  return hipGetLastError();
}

// Rows `streams[k]` of `src` into the same rows of `dst`, `floats` floats each; one workgroup column per stream (blockIdx.y), the
// row's floats spread over blockIdx.x x 256 threads. Moves data and does no arithmetic.
__global__ __launch_bounds__(256) void nam_state_rows_copy_kernel(float* __restrict__ dst, long dst_stride, const float* __restrict__ src,
                                                                  long src_stride, const int* __restrict__ streams, int floats)
{
  const int stream = streams ? streams[blockIdx.y] : (int)blockIdx.y;
  float* const D = dst + (size_t)stream * (size_t)dst_stride;
  const float* const S = src + (size_t)stream * (size_t)src_stride;
  for (int i = (int)(blockIdx.x * 256 + threadIdx.x); i < floats; i += (int)(gridDim.x * 256))
    D[i] = S[i];
}

// `streams`: n_streams stream indices in device memory (nullptr: streams 0 .. n_streams - 1), each below the row count of both
// allocations; `floats` <= both strides (the caller's check: api_launch.cpp, mix_move)
hipError_t launch_state_rows_copy(float* dst, long dst_stride, const float* src, long src_stride, const int* streams, int n_streams, int floats,
                                  hipStream_t stream)
{
  if (n_streams <= 0 || floats <= 0)
    return hipSuccess;
  if (!dst || !src || dst == src || n_streams > 65535 || floats > dst_stride || floats > src_stride)
    return hipErrorInvalidValue;
  const unsigned per_row = (unsigned)std::min((floats + 255) / 256, 64); // (up to 64 workgroups a row; a thread then takes every 16,384th float)
  hipLaunchKernelGGL(nam_state_rows_copy_kernel, dim3(per_row, (unsigned)n_streams), dim3(256), 0, stream, dst, dst_stride, src, src_stride, streams,
                     floats);
  return hipGetLastError();
}
} // namespace namhip
