// linear_index_check.cpp — a host walk of kernel_linear.hip's index arithmetic: the three kernels of a Linear launch piece, lane by
// lane, with every address asserted in range and every value computed (fmaf chains in the matrix instruction's k order), against
// a float64 convolution. No GPU: the tool to reach for before a changed kernel runs on one.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I neuralampmodelercore_amd/csrc -o linear_index_check tools/src/linear_index_check.cpp
//   ./linear_index_check          (exit 0 = every address in range and every output within 1e-5 of the convolution)
// The split rule is build_linear_plan's (plan.cpp), the geometry upload_group's (api_launch.cpp), the loops the kernels'.
#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "plan.h"

using namespace namhip;

#define CHECK(c)                                                                                                       \
  do                                                                                                                   \
  {                                                                                                                    \
    if (!(c))                                                                                                          \
    {                                                                                                                  \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);                                                     \
      std::exit(1);                                                                                                    \
    }                                                                                                                  \
  } while (0)

struct Batch
{
  LinearPlan L;
  std::vector<float> blob, hist, part;
  int n_streams, n_cols, cols_pad, hist_frames, part_frames, piece, pos = 0;
};

static Batch make(int R, int in_ch, int out_ch, int n_streams, int max_frames, unsigned seed)
{
  Batch b;
  LinearPlan& L = b.L;
  L.receptive_field = R;
  L.in_ch = in_ch;
  L.out_ch = out_ch;
  L.cols_per_stream = std::min(in_ch, out_ch);
  const int want = std::min(kLinearMaxSplits, (R + kLinearSplitTapsMin - 1) / kLinearSplitTapsMin);
  L.split_taps = ((R + want - 1) / want + kBlock - 1) / kBlock * kBlock;
  L.n_splits = (R + L.split_taps - 1) / L.split_taps;
  L.taps_off = kLinearPad;
  L.bias = 0.0123f;
  b.blob.assign((size_t)kLinearPad + (size_t)L.n_splits * L.split_taps + kLinearPad, 0.0f);
  std::srand(seed);
  for (int k = 0; k < R; k++)
    b.blob[(size_t)L.taps_off + k] = (float)((std::rand() % 2001 - 1000) / 1000.0 * std::exp(-6.0 * k / R));
  b.n_streams = n_streams;
  b.n_cols = n_streams * L.cols_per_stream;
  b.cols_pad = (b.n_cols + kLinearColTile - 1) / kLinearColTile * kLinearColTile;
  b.piece = L.piece_frames(max_frames);
  b.part_frames = (b.piece + kBlock - 1) / kBlock * kBlock;
  b.hist_frames = L.hist_frames(max_frames);
  b.hist.assign((size_t)b.hist_frames * b.cols_pad, 0.0f);
  b.part.assign((size_t)L.n_splits * b.part_frames * b.cols_pad, NAN); // (a read of a row nobody wrote shows)
  return b;
}

// one launch piece: in [stream][in_ch][stride], out [stream][out_ch][stride]
static void piece(Batch& b, const float* in, float* out, int n_frames, long stride)
{
  const LinearPlan& L = b.L;
  const int cps = L.cols_per_stream, HL = b.hist_frames, CP = b.cols_pad;
  CHECK(n_frames > 0 && n_frames <= b.part_frames && HL >= L.n_splits * L.split_taps + b.part_frames - (kBlock - 1) && b.pos >= 0 && b.pos < HL);
  const int tiles_x = CP / kLinearColTile, tiles_y = (n_frames + kBlock - 1) / kBlock;
  // nam_linear_append_kernel
  for (int bx = 0; bx < tiles_x; bx++)
    for (int by = 0; by < tiles_y; by++)
      for (int tid = 0; tid < 256; tid++)
      {
        const int col0 = bx * 32, f0 = by * 64, c = tid & 31, fr = tid >> 5;
        if (col0 + c >= b.n_cols)
          continue;
        for (int j = 0; j < 8; j++)
        {
          const int f = fr * 8 + j;
          if (f0 + f >= n_frames)
            break;
          const int col = col0 + c, s = col / cps, ch = col - s * cps;
          CHECK(s < b.n_streams && ch < L.in_ch);
          int row = b.pos + f0 + f;
          if (row >= HL)
            row -= HL;
          CHECK(row >= 0 && row < HL);
          b.hist[(size_t)row * CP + col] = in[((size_t)s * L.in_ch + ch) * stride + f0 + f];
        }
      }
  // nam_linear_kernel
  const int KS = L.split_taps;
  std::vector<float> hs((size_t)KS + 2 * kLinearPad);
  for (int bx = 0; bx < tiles_x; bx++)
    for (int split = 0; split < L.n_splits; split++)
      for (int bz = 0; bz < tiles_y; bz++)
      {
        const int col0 = bx * 32, F0 = bz * 64, t0 = split * KS;
        for (int j = 0; j < KS + 2 * kLinearPad; j++)
        {
          const int t = j - kLinearPad;
          if (t >= 0 && t < KS)
            CHECK((size_t)(L.taps_off + t0 + t) < b.blob.size());
          hs[(size_t)j] = (t >= 0 && t < KS) ? b.blob[(size_t)(L.taps_off + t0 + t)] : 0.0f;
        }
        // D[frame 0..63][column 0..31], accumulated in the instruction's order: per step, k = 0 then k = 1
        std::vector<float> D(64 * 32, 0.0f);
        int row[2], ja[2][32];
        for (int kk = 0; kk < 2; kk++)
        {
          row[kk] = b.pos + F0 - t0 - KS + kk;
          CHECK(row[kk] > -HL - 1 && row[kk] < 2 * HL);
          if (row[kk] < 0)
            row[kk] += HL;
          if (row[kk] >= HL)
            row[kk] -= HL;
          for (int i = 0; i < 32; i++)
            ja[kk][i] = i + KS + kLinearPad - kk;
        }
        const int groups = (KS + kBlock) / 16;
        CHECK(groups % 2 == 0);
        for (int g = 0; g < groups; g++)
        {
          for (int u = 0; u < 8; u++)
            for (int kk = 0; kk < 2; kk++)
            {
              int rr = row[kk] + 2 * u;
              if (rr >= HL)
                rr -= HL;
              CHECK(rr >= 0 && rr < HL);
              for (int i = 0; i < 32; i++) // lane (i, kk): A for both halves, B for column i
              {
                const int j0 = ja[kk][i] - 2 * u, j1 = j0 + 32;
                CHECK(j0 >= 0 && j1 < KS + 2 * kLinearPad);
                for (int c = 0; c < 32; c++)
                {
                  const float bv = b.hist[(size_t)rr * CP + col0 + c];
                  D[(size_t)i * 32 + c] = std::fmaf(hs[(size_t)j0], bv, D[(size_t)i * 32 + c]);
                  D[(size_t)(i + 32) * 32 + c] = std::fmaf(hs[(size_t)j1], bv, D[(size_t)(i + 32) * 32 + c]);
                }
              }
            }
          for (int kk = 0; kk < 2; kk++)
          {
            row[kk] += 16;
            if (row[kk] >= HL)
              row[kk] -= HL;
            for (int i = 0; i < 32; i++)
              ja[kk][i] -= 16;
          }
        }
        for (int r = 0; r < 64; r++)
          for (int c = 0; c < 32; c++)
          {
            const size_t at = ((size_t)split * b.part_frames + F0 + r) * CP + col0 + c;
            CHECK(at < b.part.size());
            b.part[at] = D[(size_t)r * 32 + c];
          }
      }
  // nam_linear_reduce_kernel (+ nam_linear_zero_kernel)
  for (int f = 0; f < n_frames; f++)
    for (int col = 0; col < b.n_cols; col++)
    {
      float acc = 0.0f;
      for (int s = 0; s < L.n_splits; s++)
      {
        const size_t at = ((size_t)s * b.part_frames + f) * CP + col;
        CHECK(at < b.part.size());
        acc += b.part[at];
      }
      const int s = col / cps, ch = col - s * cps;
      out[((size_t)s * L.out_ch + ch) * stride + f] = acc + L.bias;
    }
  for (int s = 0; s < b.n_streams; s++)
    for (int ch = cps; ch < L.out_ch; ch++)
      for (int f = 0; f < n_frames; f++)
        out[((size_t)s * L.out_ch + ch) * stride + f] = 0.0f;
  b.pos = (b.pos + n_frames) % HL;
}

static double run_case(int R, int in_ch, int out_ch, int n_streams, int max_frames, int total, const std::vector<int>& call_lengths)
{
  Batch b = make(R, in_ch, out_ch, n_streams, max_frames, (unsigned)R);
  const int cps = b.L.cols_per_stream;
  std::vector<float> x((size_t)n_streams * in_ch * total), y((size_t)n_streams * out_ch * total, NAN);
  for (size_t i = 0; i < x.size(); i++)
    x[i] = (float)((std::rand() % 2001 - 1000) / 1000.0);
  int at = 0, call = 0;
  while (at < total)
  {
    const int n = std::min(call_lengths[(size_t)call++ % call_lengths.size()], total - at);
    for (int p = 0; p < n; p += b.piece) // launch_linear_group
      piece(b, x.data() + at + p, y.data() + at + p, std::min(b.piece, n - p), total);
    at += n;
  }
  double worst = 0.0;
  for (int s = 0; s < n_streams; s++)
    for (int ch = 0; ch < out_ch; ch++)
      for (int f = 0; f < total; f++)
      {
        double want = 0.0;
        if (ch < cps)
        {
          want = b.L.bias;
          for (int k = 0; k < R && k <= f; k++)
            want += (double)b.blob[(size_t)b.L.taps_off + k] * x[((size_t)s * in_ch + ch) * total + f - k];
        }
        worst = std::max(worst, std::fabs(want - (double)y[((size_t)s * out_ch + ch) * total + f]));
        CHECK(ch < cps || y[((size_t)s * out_ch + ch) * total + f] == 0.0f);
      }
  std::printf("R=%d in=%d out=%d streams=%d max_frames=%d frames=%d splits=%d x %d hist=%d: max error %.3g\n", R, in_ch, out_ch, n_streams,
              max_frames, total, b.L.n_splits, b.L.split_taps, b.hist_frames, worst);
  return worst;
}

int main()
{
  double worst = 0.0;
  const std::vector<int> ragged = {1, 64, 63, 65, 17, 128, 200, 256}, blocks = {64};
  for (int R : {1, 2, 63, 64, 65, 257, 1025})
    worst = std::max(worst, run_case(R, 1, 1, 3, 64, R + 200, blocks));
  worst = std::max(worst, run_case(257, 1, 1, 4, 256, 3000, ragged)); // wraps the ring (hist = 896) three times
  worst = std::max(worst, run_case(257, 1, 1, 33, 256, 1500, {1500})); // a launch cut into pieces; a partial column tile
  worst = std::max(worst, run_case(65, 2, 3, 17, 64, 300, ragged)); // columns straddle tiles; a zero output channel
  worst = std::max(worst, run_case(65, 3, 2, 5, 700, 1500, {700, 3})); // max_frames above the piece cap
  worst = std::max(worst, run_case(4099, 1, 1, 1, 64, 4099 + 130, blocks));
  if (!(worst < 1e-5))
  {
    std::fprintf(stderr, "FAILED: max error %.3g\n", worst);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
