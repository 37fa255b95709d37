// linear_container_check — a SlimmableContainer whose submodels are all Linear (one impulse response at several sizes) through the C++
// adapter, unchanged: nam::get_dsp(path) returns an object that casts to nam::SlimmableModel; three nam::DSP instances run three of
// the sizes (the smallest, the second largest, the largest) in 64-frame buffers and are compared with a direct convolution on the
// host; then one nam::BatchDSP runs the three sizes side by side, one stream each (SetSlimmableSize per stream), and must produce
// the instances' bits.
// The bound of the host comparison: float32 taps and input, summed in ANY order with or without fused multiply-adds, differ from
// the exact sum by at most (R + 1) u sum |h[k] x[n - k]|, u = 2^-24 (the a-priori bound of recursive summation); the bias adds one
// rounding. The check uses (R + 2) u (sum |h| max |x| + |bias|).
// The taps are read from the file's "weights" arrays (the container's own is empty; every submodel's holds its R taps and the bias).
// Usage: linear_container_check <container.nam> [n_frames = 2048]. Prints "all checks passed" and exits 0, or says what failed.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <vector>

#include "NAM/get_dsp.h"
#include "NAM/slimmable.h"

static std::vector<std::vector<float>> weight_arrays(const std::string& text)
{
  std::vector<std::vector<float>> out;
  const std::string key = "\"weights\"";
  for (size_t at = text.find(key); at != std::string::npos; at = text.find(key, at + key.size()))
  {
    const size_t open = text.find('[', at), close = text.find(']', at);
    if (open == std::string::npos || close == std::string::npos || close < open)
      break;
    std::vector<float> w;
    const char* p = text.c_str() + open + 1;
    const char* const end = text.c_str() + close;
    while (p < end)
    {
      char* next = nullptr;
      const double v = std::strtod(p, &next);
      if (next == p)
        break;
      w.push_back((float)v);
      p = next;
      while (p < end && (*p == ',' || *p == ' ' || *p == '\n'))
        p++;
    }
    if (!w.empty())
      out.push_back(std::move(w));
  }
  return out;
}

int main(int argc, char** argv)
{
  if (argc < 2)
  {
    std::fprintf(stderr, "usage: linear_container_check <container.nam> [n_frames]\n");
    return 2;
  }
  const int n = argc > 2 ? std::atoi(argv[2]) : 2048;
  constexpr int kBlock = 64;
  int failures = 0;
  try
  {
    std::ifstream f(argv[1]);
    std::stringstream ss;
    ss << f.rdbuf();
    const std::vector<std::vector<float>> subs = weight_arrays(ss.str());
    std::unique_ptr<nam::DSP> probe = nam::get_dsp(std::filesystem::path(argv[1]));
    nam::SlimmableModel* slim = dynamic_cast<nam::SlimmableModel*>(probe.get());
    if (!slim)
    {
      std::fprintf(stderr, "linear_container_check: get_dsp did not return a nam::SlimmableModel\n");
      return 1;
    }
    const std::vector<double> bp = slim->GetSlimmableSizeBreakpoints();
    const int W = (int)bp.size() + 1;
    std::printf("submodels %d in_channels %d out_channels %d prewarm_samples %d\n", W, probe->NumInputChannels(), probe->NumOutputChannels(),
                probe->GetPrewarmSamples());
    if ((int)subs.size() != W || W < 3 || probe->NumInputChannels() != 1 || probe->NumOutputChannels() != 1 || probe->GetPrewarmSamples() != 0)
    {
      std::fprintf(stderr, "linear_container_check: %d weight arrays for %d submodels (at least three, mono, no prewarm expected)\n", (int)subs.size(), W);
      return 1;
    }
    auto ratio_of = [&](int w) { return w == W - 1 ? 1.0 : 0.5 * ((w ? bp[(size_t)w - 1] : 0.0) + bp[(size_t)w]); };
    const int sizes[3] = {0, W - 2, W - 1};

    // three streams of input: two tones each, another pair per stream
    std::vector<float> x((size_t)3 * n);
    const double two_pi = 6.283185307179586476925286766559;
    for (int s = 0; s < 3; s++)
      for (int i = 0; i < n; i++)
      {
        const double t = (double)i / 48000.0;
        x[(size_t)s * n + i] = (float)(0.25 * std::sin(two_pi * 220.0 * (1 + s) * t) + 0.10 * std::sin(two_pi * (1230.0 + 77.0 * s) * t));
      }

    // 1. three nam::DSP instances at three sizes against the direct convolution
    std::vector<float> y_single((size_t)3 * n);
    for (int k = 0; k < 3; k++)
    {
      const int w = sizes[k];
      std::unique_ptr<nam::DSP> dsp = nam::get_dsp(std::filesystem::path(argv[1]));
      dynamic_cast<nam::SlimmableModel&>(*dsp).SetSlimmableSize(ratio_of(w));
      dsp->Reset(48000.0, kBlock);
      std::vector<NAM_SAMPLE> in((size_t)n), out((size_t)n, NAM_SAMPLE(0));
      for (int i = 0; i < n; i++)
        in[(size_t)i] = (NAM_SAMPLE)x[(size_t)k * n + i];
      for (int at = 0; at < n; at += kBlock)
      {
        NAM_SAMPLE* pi[1] = {in.data() + at};
        NAM_SAMPLE* po[1] = {out.data() + at};
        dsp->process(pi, po, n - at < kBlock ? n - at : kBlock);
      }
      const std::vector<float>& h = subs[(size_t)w];
      const int R = (int)h.size() - 1; // (the fixture's submodels have a bias)
      double sum_h = 0.0, max_x = 0.0, worst = 0.0;
      for (int t = 0; t < R; t++)
        sum_h += std::fabs((double)h[(size_t)t]);
      for (int i = 0; i < n; i++)
        max_x = std::fmax(max_x, std::fabs((double)x[(size_t)k * n + i]));
      const double bound = (R + 2) * std::ldexp(1.0, -24) * (sum_h * max_x + std::fabs((double)h[(size_t)R]));
      for (int i = 0; i < n; i++)
      {
        double acc = 0.0;
        for (int t = 0; t < R && t <= i; t++)
          acc += (double)h[(size_t)t] * (double)x[(size_t)k * n + i - t];
        acc += (double)h[(size_t)R];
        worst = std::fmax(worst, std::fabs((double)out[(size_t)i] - acc));
        y_single[(size_t)k * n + i] = (float)out[(size_t)i];
      }
      std::printf("size %d: %d taps, max |y - convolution| = %.3e, bound %.3e\n", w, R, worst, bound);
      if (!(worst <= bound))
      {
        std::printf("FAILED: size %d is outside the bound\n", w);
        failures++;
      }
    }

    // 2. the same three through one BatchDSP, a size per stream
    {
      nam_hip_model* raw = nullptr;
      nam::detail::check(nam_hip_model_load(argv[1], 0, &raw));
      std::shared_ptr<nam_hip_model> model(raw, nam::detail::ModelDeleter());
      nam::BatchDSP batch(model, 3);
      batch.Reset(48000.0, kBlock);
      if (!batch.IsSlimmable())
      {
        std::printf("FAILED: the BatchDSP is not slimmable\n");
        failures++;
      }
      for (int k = 0; k < 3; k++)
        batch.SetSlimmableSize(&k, 1, ratio_of(sizes[k]));
      std::vector<float> in((size_t)3 * kBlock), out((size_t)3 * kBlock);
      long differing = 0;
      for (int at = 0; at < n; at += kBlock)
      {
        const int m = n - at < kBlock ? n - at : kBlock;
        for (int k = 0; k < 3; k++)
          std::memcpy(in.data() + (size_t)k * m, x.data() + (size_t)k * n + at, (size_t)m * sizeof(float));
        batch.process_batch(in.data(), out.data(), m);
        for (int k = 0; k < 3; k++)
          differing += std::memcmp(out.data() + (size_t)k * m, y_single.data() + (size_t)k * n + at, (size_t)m * sizeof(float)) != 0;
      }
      std::printf("BatchDSP with a size per stream: %ld buffers differ from the single instances\n", differing);
      if (differing)
      {
        std::printf("FAILED: the batch and the single instances differ\n");
        failures++;
      }
    }
  }
  catch (const std::exception& e)
  {
    std::fprintf(stderr, "linear_container_check: %s\n", e.what());
    return 1;
  }
  if (failures)
    return 1;
  std::printf("all checks passed\n");
  return 0;
}
