// linear_check — a Linear .nam file (an impulse response, reference NAM/linear.cpp) through the C++ adapter, unchanged:
// nam::get_dsp(path), the nam::DSP getters, Reset, and process() in 64-frame buffers on the two-tone of the parity tests
// (0.25 sin(2 pi 220 t) + 0.10 sin(2 pi 1230 t) at 48 kHz). Prints the getters as "key value" lines, then "y <n>" and the n output
// samples, one per line with 9 significant digits (a float32 round trip); the caller compares them with its own yardstick
// (tests/test_gpu_linear.py). Exit code 0 = loaded as Linear-shaped (1 in / 1 out, no prewarm) and rendered.
// Usage: linear_check <model.nam> [n_frames = 768]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "NAM/get_dsp.h"

int main(int argc, char** argv)
{
  if (argc < 2)
  {
    std::fprintf(stderr, "usage: linear_check <model.nam> [n_frames]\n");
    return 2;
  }
  const int n = argc > 2 ? std::atoi(argv[2]) : 768;
  constexpr int kBlock = 64;
  try
  {
    std::unique_ptr<nam::DSP> dsp = nam::get_dsp(std::filesystem::path(argv[1]));
    std::printf("in_channels %d\nout_channels %d\nprewarm_samples %d\nsample_rate %.17g\nhas_loudness %d\n", dsp->NumInputChannels(),
                dsp->NumOutputChannels(), dsp->GetPrewarmSamples(), dsp->GetExpectedSampleRate(), dsp->HasLoudness() ? 1 : 0);
    if (dsp->NumInputChannels() != 1 || dsp->NumOutputChannels() != 1 || dsp->GetPrewarmSamples() != 0)
    {
      std::fprintf(stderr, "linear_check: not a mono Linear model\n");
      return 1;
    }
    dsp->Reset(48000.0, kBlock);
    std::vector<NAM_SAMPLE> x((size_t)n), y((size_t)n, NAM_SAMPLE(0));
    const double two_pi = 6.283185307179586476925286766559;
    for (int i = 0; i < n; i++)
    {
      const double t = (double)i / 48000.0;
      x[(size_t)i] = (NAM_SAMPLE)(float)(0.25 * std::sin(two_pi * 220.0 * t) + 0.10 * std::sin(two_pi * 1230.0 * t));
    }
    for (int at = 0; at < n; at += kBlock)
    {
      NAM_SAMPLE* in[1] = {x.data() + at};
      NAM_SAMPLE* out[1] = {y.data() + at};
      dsp->process(in, out, n - at < kBlock ? n - at : kBlock);
    }
    std::printf("y %d\n", n);
    for (int i = 0; i < n; i++)
      std::printf("%.9g\n", (double)y[(size_t)i]);
  }
  catch (const std::exception& e)
  {
    std::fprintf(stderr, "linear_check: %s\n", e.what());
    return 1;
  }
  return 0;
}
