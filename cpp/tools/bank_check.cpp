// bank_check — exercises nam::ModelBank and the bank form of nam::BatchDSP (cpp/NAM/dsp.h) on the GPU:
//   * a bank batch whose stream s runs member s % n renders, bit for bit, what one-model BatchDSPs of the members render for
//     the same input (blocking process_batch calls of 64 frames, after Reset with prewarm);
//   * SetStreamModel moves a stream to another member: from then on it renders what a freshly reset one-model batch of
//     that member renders for the remaining input, and the streams that stayed are untouched;
//   * a bank over models that cannot share a launch throws std::runtime_error naming the member.
// Usage: bank_check <a.nam> <b.nam> [<c.nam> ...] [--refuse <other.nam>]      exit code 0 = every check passed
#include <cmath>
#include <cstdio>
#include <cstring>

#include "NAM/get_dsp.h"

namespace
{
int failures = 0;
void expect(bool ok, const char* what)
{
  std::printf("%s %s\n", ok ? "ok  " : "FAIL", what);
  if (!ok)
    failures++;
}
constexpr int kBlock = 64;
// input of stream s, frame t
float signal(int s, int t)
{
  return 0.3f * std::sin(0.05f * (float)t * (1.f + 0.1f * (float)s)) + 0.1f * std::sin(0.31f * (float)t + (float)s);
}
// blocks [b0, b1) of every stream through `dsp`; returns [stream][(b1 - b0) * 64]
std::vector<std::vector<float>> render(nam::BatchDSP& dsp, int n_streams, int b0, int b1, const std::vector<int>& stream_of_row)
{
  std::vector<std::vector<float>> out((size_t)n_streams);
  std::vector<float> in((size_t)n_streams * kBlock), y((size_t)n_streams * kBlock);
  for (int b = b0; b < b1; b++)
  {
    for (int r = 0; r < n_streams; r++)
      for (int i = 0; i < kBlock; i++)
        in[(size_t)r * kBlock + i] = signal(stream_of_row[(size_t)r], b * kBlock + i);
    dsp.process_batch(in.data(), y.data(), kBlock);
    for (int r = 0; r < n_streams; r++)
      out[(size_t)r].insert(out[(size_t)r].end(), y.begin() + (size_t)r * kBlock, y.begin() + (size_t)(r + 1) * kBlock);
  }
  return out;
}
} // namespace

int main(int argc, char** argv)
{
  std::vector<std::string> paths;
  std::string refuse;
  for (int i = 1; i < argc; i++)
  {
    if (!std::strcmp(argv[i], "--refuse") && i + 1 < argc)
      refuse = argv[++i];
    else
      paths.push_back(argv[i]);
  }
  if (paths.size() < 2)
  {
    std::fprintf(stderr, "usage: bank_check <a.nam> <b.nam> [<c.nam> ...] [--refuse <other.nam>]\n");
    return 2;
  }
  try
  {
    nam::activations::Activation::enable_fast_tanh();
    const nam::ModelBank bank = nam::ModelBank::FromFiles(paths);
    const int n_members = bank.size();
    expect(n_members == (int)paths.size(), "ModelBank::FromFiles holds every model");
    const int n_streams = 3 * n_members + 1, n_blocks = 8, swap_at = 3;
    std::vector<int> members((size_t)n_streams), all((size_t)n_streams);
    for (int s = 0; s < n_streams; s++)
    {
      members[(size_t)s] = s % n_members;
      all[(size_t)s] = s;
    }
    nam::BatchDSP banked(bank, members);
    banked.Reset(48000.0, kBlock);
    const auto first = render(banked, n_streams, 0, swap_at, all);
    // one-model batches of every member, fed the streams bound to it
    bool equal = true, finite = true;
    std::vector<std::vector<std::vector<float>>> rest_by_member((size_t)n_members);
    for (int m = 0; m < n_members; m++)
    {
      std::vector<int> rows;
      for (int s = 0; s < n_streams; s++)
        if (members[(size_t)s] == m)
          rows.push_back(s);
      nam::BatchDSP single(bank.model(m), (int)rows.size());
      single.Reset(48000.0, kBlock);
      const auto want = render(single, (int)rows.size(), 0, swap_at, rows);
      for (size_t r = 0; r < rows.size(); r++)
      {
        equal = equal && want[r] == first[(size_t)rows[r]];
        for (float v : want[r])
          finite = finite && std::isfinite(v);
      }
      rest_by_member[(size_t)m] = render(single, (int)rows.size(), swap_at, n_blocks, rows);
    }
    expect(finite, "outputs are finite");
    expect(equal, "every stream of the bank batch == the one-model batch of its member, bit for bit");

    // stream 1 moves to the last member
    const int moved = 1, to = n_members - 1;
    banked.SetStreamModel(&moved, 1, to);
    expect(banked.GetStreamModel(moved) == to && nam_hip_batch_get_stream_model(banked.GetBatchHandle(), moved) == to,
           "SetStreamModel is reported by GetStreamModel / nam_hip_batch_get_stream_model");
    const auto rest = render(banked, n_streams, swap_at, n_blocks, all);
    {
      nam::BatchDSP fresh(bank.model(to), 1);
      fresh.Reset(48000.0, kBlock);
      const auto want = render(fresh, 1, swap_at, n_blocks, std::vector<int>{moved});
      expect(want[0] == rest[(size_t)moved], "the moved stream == a freshly reset one-model batch of the new member, bit for bit");
    }
    bool untouched = true;
    for (int m = 0; m < n_members; m++)
    {
      int r = 0;
      for (int s = 0; s < n_streams; s++)
        if (members[(size_t)s] == m)
        {
          if (s != moved)
            untouched = untouched && rest_by_member[(size_t)m][(size_t)r] == rest[(size_t)s];
          r++;
        }
    }
    expect(untouched, "every other stream runs on as if nothing had happened, bit for bit");
    bool threw = false;
    try
    {
      banked.SetStreamModel(&moved, 1, n_members);
    }
    catch (const std::runtime_error&)
    {
      threw = true;
    }
    expect(threw && banked.GetStreamModel(moved) == to, "a member out of range throws and changes nothing");

    if (!refuse.empty())
    {
      threw = false;
      try
      {
        nam::ModelBank::FromFiles({paths[0], refuse});
      }
      catch (const std::runtime_error& e)
      {
        threw = std::strstr(e.what(), "member 1") != nullptr;
      }
      expect(threw, "a model that cannot share the launch is refused, naming member 1");
    }
  }
  catch (const std::exception& e)
  {
    std::printf("FAIL exception: %s\n", e.what());
    return 1;
  }
  std::printf("%s\n", failures ? "bank_check: FAILED" : "bank_check: all checks passed");
  return failures ? 1 : 0;
}
