// stream_state_check — the stream slots of nam::BatchDSP (cpp/NAM/dsp.h: RestartStreams, GetStreamState, SetStreamState) on the GPU,
// once through the C++ adapter (blocking process_batch calls of 64 frames, after Reset with prewarm):
//   * move: the blob of stream 4 of a 5-stream BatchDSP after three buffers, set into stream 0 of a 3-stream BatchDSP that has
//     processed one unrelated buffer: from then on that stream renders, bit for bit, what the source stream renders, and the
//     destination's other streams run on as if nothing had happened;
//   * restart: streams restarted on the source render what a freshly built BatchDSP renders for the same input;
//   * a corrupted blob throws std::runtime_error and changes nothing.
// Usage: stream_state_check <model.nam>      exit code 0 = every check passed
#include <cmath>
#include <cstdio>

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
// input of signal s, frame t
float signal(int s, int t)
{
  return 0.3f * std::sin(0.05f * (float)t * (1.f + 0.1f * (float)s)) + 0.1f * std::sin(0.31f * (float)t + (float)s);
}
// blocks [b0, b1) through `dsp`, row r fed signal signal_of_row[r]; returns [row][(b1 - b0) * 64]
std::vector<std::vector<float>> render(nam::BatchDSP& dsp, int b0, int b1, const std::vector<int>& signal_of_row)
{
  const int n = (int)signal_of_row.size();
  std::vector<std::vector<float>> out((size_t)n);
  std::vector<float> in((size_t)n * kBlock), y((size_t)n * kBlock);
  for (int b = b0; b < b1; b++)
  {
    for (int r = 0; r < n; r++)
      for (int i = 0; i < kBlock; i++)
        in[(size_t)r * kBlock + i] = signal(signal_of_row[(size_t)r], b * kBlock + i);
    dsp.process_batch(in.data(), y.data(), kBlock);
    for (int r = 0; r < n; r++)
      out[(size_t)r].insert(out[(size_t)r].end(), y.begin() + (size_t)r * kBlock, y.begin() + (size_t)(r + 1) * kBlock);
  }
  return out;
}
} // namespace

int main(int argc, char** argv)
{
  if (argc < 2)
  {
    std::fprintf(stderr, "usage: stream_state_check <model.nam>\n");
    return 2;
  }
  try
  {
    nam::activations::Activation::enable_fast_tanh();
    const std::shared_ptr<nam_hip_model> model = nam::ModelBank::FromFiles({argv[1]}).model(0);
    const std::vector<int> five{0, 1, 2, 3, 4}, three{4, 5, 6}, unrelated{7, 8, 9};
    nam::BatchDSP a(model, 5);
    a.Reset(48000.0, kBlock);
    render(a, 0, 3, five);
    const std::vector<unsigned char> blob = a.GetStreamState(4);
    expect(blob.size() > 80, "GetStreamState returns a blob");
    const auto a_rest = render(a, 3, 6, five);

    // the destination with the blob, and the same destination left alone
    nam::BatchDSP d(model, 3), w(model, 3);
    for (nam::BatchDSP* b : {&d, &w})
    {
      b->Reset(48000.0, kBlock);
      render(*b, 0, 1, unrelated);
    }
    std::vector<unsigned char> bad = blob;
    bad[bad.size() / 2] ^= 0x20;
    bool threw = false;
    try
    {
      d.SetStreamState(1, bad);
    }
    catch (const std::runtime_error&)
    {
      threw = true;
    }
    expect(threw, "a corrupted blob throws");
    d.SetStreamState(0, blob);
    const auto d_rest = render(d, 3, 6, three), w_rest = render(w, 3, 6, three);
    bool finite = true;
    for (float v : d_rest[0])
      finite = finite && std::isfinite(v);
    expect(finite, "outputs are finite");
    expect(d_rest[0] == a_rest[4], "the moved stream == the source stream, bit for bit");
    expect(d_rest[0] != w_rest[0], "... and not what the slot would have rendered");
    expect(d_rest[1] == w_rest[1] && d_rest[2] == w_rest[2], "the destination's other streams run on as if nothing had happened, bit for bit");

    // streams 1 and 3 of the source start over
    const int ids[2] = {1, 3};
    a.RestartStreams(ids, 2, true);
    const auto a_new = render(a, 0, 3, five);
    nam::BatchDSP fresh(model, 5);
    fresh.Reset(48000.0, kBlock);
    const auto want = render(fresh, 0, 3, five);
    expect(a_new[1] == want[1] && a_new[3] == want[3], "restarted streams == a freshly built BatchDSP, bit for bit");
    expect(a_new[0] != want[0], "... the others kept their state");
  }
  catch (const std::exception& e)
  {
    std::printf("FAIL exception: %s\n", e.what());
    return 1;
  }
  std::printf("%s\n", failures ? "stream_state_check: FAILED" : "stream_state_check: all checks passed");
  return failures ? 1 : 0;
}
