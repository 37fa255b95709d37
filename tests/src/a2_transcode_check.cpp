// a2_transcode_check.cpp — csrc/a2_transcode.h on the CPU (tests/test_a2_transcode.py; no device: plan.h, the loader and the
// planner alone). For the container given (tests/golden/models/A2.nam): every narrower submodel's zero-padded plan equals the
// largest submodel's layout field by field and differs from it in weights only where the padding says; the transcode table between
// the submodel's nam_wn_reg_kernel state and the padded rings passes its own check, covers every ring of both plans exactly once,
// and — walked here the way kernel_a2_transcode.hip walks it — carries a state there and back without losing a float, fills the
// padded channels with zeros and keeps every write position. Tables that must be refused are refused.
#include "a2_transcode.h"

#include <cstdio>
#include <cstdlib>

using namespace namhip;

static int g_failures = 0;
#define EXPECT(cond, ...)                                                                                                          \
  do                                                                                                                               \
  {                                                                                                                                \
    if (!(cond))                                                                                                                   \
    {                                                                                                                              \
      std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond);                                                                \
      std::printf(__VA_ARGS__);                                                                                                    \
      std::printf("\n");                                                                                                           \
      g_failures++;                                                                                                                \
    }                                                                                                                              \
  } while (0)

// the kernel's walk (kernel_a2_transcode.hip), one stream
static void transcode(const A2Transcode& t, std::vector<float>& a2, std::vector<float>& wr, bool to_padded)
{
  for (const A2XcRing& r : t.rings)
  {
    for (int i = 0; i < r.R; i++)
      for (int c = 0; c < r.a2_ch; c++)
      {
        float& A = a2.at((size_t)r.a2_off + (size_t)i * r.a2_ch + c);
        if (to_padded)
          A = c < r.wr_ch ? wr.at((size_t)r.wr_off[c] + (size_t)i * r.wr_gs[c]) : 0.0f;
        else if (c < r.wr_ch)
          wr.at((size_t)r.wr_off[c] + (size_t)i * r.wr_gs[c]) = A;
      }
    if (to_padded)
      std::memcpy(&a2.at((size_t)r.ring_id), &wr.at((size_t)r.slot), 4);
    else
      std::memcpy(&wr.at((size_t)r.slot), &a2.at((size_t)r.ring_id), 4);
  }
}

int main(int argc, char** argv)
{
  if (argc < 2)
  {
    std::printf("usage: a2_transcode_check CONTAINER.nam\n");
    return 2;
  }
  LoadOptions lo;
  const std::shared_ptr<ModelSpec> spec = load_nam_file(argv[1], lo);
  EXPECT(spec->arch == ARCH_CONTAINER && spec->submodels.size() >= 2, "not a container of several submodels");
  if (g_failures)
    return 1;
  WrShapeSet set;
  std::vector<Plan> plans;
  for (const auto& sm : spec->submodels)
    plans.push_back(build_plan(*sm, &set));
  const Plan& full = plans.back();
  EXPECT(full.a1.valid && full.a1.kt_ok && full.a1.kp_ok, "the largest submodel is not nam_kq_kernel's topology");
  int n_checked = 0;
  for (size_t s = 0; s + 1 < plans.size(); s++)
  {
    const Plan& narrow = plans[s];
    Plan padded;
    std::string why;
    const bool ok = build_a2_padded_plan(spec->submodels[s]->wavenet, full, padded, why);
    EXPECT(ok, "submodel %zu: %s", s, why.c_str());
    if (!ok)
      continue;
    // 1. the layout, field by field (and the comparison is not vacuous: a moved ring is named)
    EXPECT(a2_layout_difference(padded, full).empty(), "%s", a2_layout_difference(padded, full).c_str());
    EXPECT(padded.blob.size() == full.blob.size() && padded.state_floats == full.state_floats, "sizes");
    {
      Plan moved = padded;
      moved.a1.arr[0].ring_off[3] += 8;
      EXPECT(a2_layout_difference(moved, full).find("ring_off") != std::string::npos, "a moved ring went unnoticed");
      moved = padded;
      moved.a1.kq_w_off += 64;
      EXPECT(a2_layout_difference(moved, full).find("kq_w_off") != std::string::npos, "a moved weight block went unnoticed");
    }
    // 2. the padding is exact: in nam_kq_kernel's weight block every tile entry of a padded output row or input column, every
    // padded constant and the padded rechannel entries are zero (kernel_kq.hip: tiles [lane % 4][h][c] = W[4 h + lane % 4][c])
    {
      const int C = padded.a1.arr[0].channels, Cn = narrow.a1.valid ? narrow.a1.arr[0].channels : spec->submodels[s]->wavenet.arrays[0].channels;
      const A1Array& A = padded.a1.arr[0];
      int n_taps = A.head_k;
      for (int l = 0; l < A.n_layers; l++)
        n_taps += A.ksize[l];
      const int n_tiles = n_taps + A.n_layers, n_jobs = A.n_layers + 1;
      const float* const w = padded.blob.data() + padded.a1.kq_w_off;
      long nonzero_real = 0;
      for (int t = 0; t < n_tiles; t++)
        for (int i = 0; i < 4; i++)
          for (int h = 0; h < 2; h++)
            for (int c = 0; c < C; c++)
            {
              const float v = w[(size_t)t * 64 + i * 16 + h * 8 + c];
              if (4 * h + i >= Cn || c >= Cn)
                EXPECT(v == 0.0f, "tile %d row %d column %d is %g", t, 4 * h + i, c, (double)v);
              else
                nonzero_real += v != 0.0f;
            }
      EXPECT(nonzero_real > 0, "no weights at all");
      for (int j = 0; j < n_jobs; j++)
        for (int k = 0; k < 3; k++)
          for (int c = Cn; c < C; c++)
            EXPECT(w[(size_t)n_tiles * 64 + j * 24 + k * 8 + c] == 0.0f, "job %d constant %d channel %d", j, k, c);
      for (int c = Cn; c < C; c++)
        EXPECT(w[(size_t)n_tiles * 64 + n_jobs * 24 + c] == 0.0f, "rechannel entry %d", c);
    }
    // 3. the table
    const A2Transcode t = build_a2_transcode(narrow, padded);
    EXPECT(t.ok, "%s", t.why.c_str());
    EXPECT(a2_transcode_check(t).empty(), "%s", a2_transcode_check(t).c_str());
    if (!t.ok)
      continue;
    EXPECT((int)t.rings.size() == full.a1.n_rings && (int)t.rings.size() == narrow.wr.n_layers, "%zu rings, %d, %d", t.rings.size(),
           full.a1.n_rings, narrow.wr.n_layers);
    long wr_named = 0, a2_named = 0;
    for (const A2XcRing& r : t.rings)
    {
      wr_named += (long)r.R * r.wr_ch;
      a2_named += (long)r.R * r.a2_ch;
      EXPECT(r.R == full.a1.ring_len_by_id[r.ring_id], "ring %d length", r.ring_id);
    }
    // every float of the narrow ring area but its alignment padding, every float of the padded state behind the position table
    EXPECT(wr_named <= narrow.wr.hist_floats && wr_named + 4 * (long)t.rings.size() > narrow.wr.hist_floats, "narrow coverage %ld of %d",
           wr_named, narrow.wr.hist_floats);
    EXPECT(a2_named + kBlock <= full.state_floats && a2_named + 2 * kBlock > full.state_floats, "padded coverage %ld of %d", a2_named,
           full.state_floats);
    // 4. there and back, at odd positions
    std::vector<float> wr((size_t)narrow.state_floats), a2((size_t)full.state_floats, -7.0f);
    for (size_t i = 0; i < wr.size(); i++)
      wr[i] = (float)(i + 1);
    for (const A2XcRing& r : t.rings)
    {
      const int32_t pos = (17 * (r.slot + 3)) % r.R;
      std::memcpy(&wr[(size_t)r.slot], &pos, 4);
    }
    const std::vector<float> wr0 = wr;
    transcode(t, a2, wr, true);
    for (const A2XcRing& r : t.rings)
    {
      EXPECT(std::memcmp(&a2[(size_t)r.ring_id], &wr0[(size_t)r.slot], 4) == 0, "position of ring %d", r.ring_id);
      for (int i = 0; i < r.R; i++)
        for (int c = 0; c < r.a2_ch; c++)
        {
          const float v = a2[(size_t)r.a2_off + (size_t)i * r.a2_ch + c];
          if (c >= r.wr_ch)
            EXPECT(v == 0.0f, "padded channel %d of ring %d row %d holds %g", c, r.ring_id, i, (double)v);
          else
            EXPECT(v == wr0[(size_t)r.wr_off[c] + (size_t)i * r.wr_gs[c]], "ring %d row %d channel %d", r.ring_id, i, c);
        }
    }
    std::fill(wr.begin(), wr.end(), -3.0f);
    transcode(t, a2, wr, false);
    long restored = 0;
    for (const A2XcRing& r : t.rings)
    {
      EXPECT(std::memcmp(&wr[(size_t)r.slot], &wr0[(size_t)r.slot], 4) == 0, "position of slot %d", r.slot);
      for (int c = 0; c < r.wr_ch; c++)
        for (int i = 0; i < r.R; i++, restored++)
          EXPECT(wr[(size_t)r.wr_off[c] + (size_t)i * r.wr_gs[c]] == wr0[(size_t)r.wr_off[c] + (size_t)i * r.wr_gs[c]], "slot %d", r.slot);
    }
    EXPECT(restored == wr_named, "restored %ld of %ld", restored, wr_named);
    const std::vector<float> a2_0 = a2;
    transcode(t, a2, wr, true); // padded -> narrow -> padded: the same image
    EXPECT(a2 == a2_0, "the padded image changed on the way back in");
    // 5. refusals
    {
      A2Transcode bad = t;
      bad.rings[2].a2_off = full.state_floats - 8;
      EXPECT(!a2_transcode_check(bad).empty(), "a ring beyond the padded state passed");
      bad = t;
      bad.rings[1].wr_off[0] = bad.rings[0].wr_off[0];
      EXPECT(!a2_transcode_check(bad).empty(), "two rings on one narrow row passed");
      bad = t;
      bad.rings[5].slot = bad.rings[4].slot;
      EXPECT(!a2_transcode_check(bad).empty(), "a slot named twice passed");
      bad = t;
      bad.wr_state_floats = narrow.wr.hist_floats / 2;
      EXPECT(!a2_transcode_check(bad).empty(), "a narrow row beyond its state passed");
      Plan other = narrow;
      other.wr.ok = false;
      EXPECT(!build_a2_transcode(other, padded).ok, "a plan without a nam_wn_reg_kernel plan was taken");
      other = padded;
      other.a1.arr[0].ring_len[6] += 1;
      EXPECT(!build_a2_transcode(narrow, other).ok, "rings of different lengths were matched");
    }
    std::printf("submodel %zu: %zu rings, %ld narrow floats <-> %ld padded floats\n", s, t.rings.size(), wr_named, a2_named);
    n_checked++;
  }
  EXPECT(n_checked >= 1, "no submodel was checked");
  // the largest submodel itself is not narrower than itself
  {
    Plan p;
    std::string why;
    EXPECT(!build_a2_padded_plan(spec->submodels.back()->wavenet, full, p, why) && !why.empty(), "the largest submodel was padded");
  }
  if (g_failures)
  {
    std::printf("a2_transcode_check: %d failure(s)\n", g_failures);
    return 1;
  }
  std::printf("a2_transcode_check: ok\n");
  return 0;
}
