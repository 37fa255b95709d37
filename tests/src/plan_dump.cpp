// plan_dump.cpp — everything the planner decides, one line per plan (tests/test_plan_pin.py; profiles/plan_wr/README.md). No device:
// plan.h alone. For every .nam path given, at fast_tanh 0 and 1, with and without a shape set on offer, the plans as
// api_launch.cpp: build_model enumerates them (the widths of a slimmable WaveNet, the submodels of a container, else the model):
// nam_wn_reg_kernel's plan field by field with hashes of its blob / ops / run records, the rest of the plan as its description and
// two hashes, and per model the shape set (header texts, programs). A1Plan is not hashed raw: its padding bytes are not defined.
#include "plan.h"

#include <algorithm>
#include <cstdio>
#include <string>

using namespace namhip;

template <class T>
static unsigned long long hash_of(const std::vector<T>& v)
{
  return wr_hash(v.data(), v.size() * sizeof(T), wr_hash_seed);
}

static std::string one_line(std::string s)
{
  std::replace(s.begin(), s.end(), '\n', ' ');
  return s;
}

static void dump_plan(const char* name, int ft, int shapes, size_t i, const Plan& p)
{
  const WrPlan& w = p.wr;
  int n_type[8] = {0}, film_layers = 0, post_rings = 0;
  for (const WrOp& o : w.ops)
  {
    if (o.type >= 0 && o.type < 8)
      n_type[o.type]++;
    film_layers += o.type == WR_LAYER && o.pad[1] != 0;
    post_rings += o.type == WR_POST_HEAD && o.ring > 0;
  }
  std::printf("plan %s ft=%d shapes=%d i=%zu ok=%d jit=%d program=%d n_layers=%d has_layers=%d has_runs=%d has_rt_layers=%d "
              "state_floats=%d hist_floats=%d lds_bytes=%d tab_rows=%d n_rows=%d tab_pf=%d n_pf=%d tab_ring=%d tab_ops=%d "
              "split_op=%d,%d,%d,%d structure_key=%016llx wr_blob=%zu:%016llx wr_ops=%zu:%016llx run_recs=%zu:%016llx "
              "n_layer=%d n_run=%d n_end_k=%d n_post=%d n_post_ring=%d n_set_cond=%d n_film_matrix=%d "
              "describe=[%s] blob=%016llx ops=%016llx why=[%s]\n",
              name, ft, shapes, i, (int)w.ok, (int)w.jit, w.program, w.n_layers, (int)w.has_layers, (int)w.has_runs, (int)w.has_rt_layers,
              w.state_floats, w.hist_floats, w.lds_bytes, w.tab_rows, w.n_rows, w.tab_pf, w.n_pf, w.tab_ring, w.tab_ops, w.split_op[0],
              w.split_op[1], w.split_op[2], w.split_op[3], w.structure_key, w.blob.size(), hash_of(w.blob), w.ops.size(), hash_of(w.ops),
              w.run_recs.size(), hash_of(w.run_recs), n_type[WR_LAYER], n_type[WR_RUN], n_type[WR_ARRAY_END_K], n_type[WR_POST_HEAD],
              post_rings, n_type[WR_SET_COND], film_layers, one_line(p.describe()).c_str(), hash_of(p.blob), hash_of(p.ops),
              one_line(w.why).c_str());
}

// api_launch.cpp: build_model, without the device
static std::vector<Plan> plans_of(const ModelSpec& spec, WrShapeSet* js)
{
  std::vector<Plan> plans;
  if (spec.arch == ARCH_WAVENET && spec.wavenet.slimmable)
  {
    std::vector<double> probes;
    double lo = 0.0;
    for (double x : slimmable_breakpoints(spec.wavenet))
    {
      probes.push_back(0.5 * (lo + x));
      lo = x;
    }
    probes.push_back(0.5 * (lo + 1.0));
    probes.push_back(1.0);
    std::vector<std::vector<int>> widths;
    for (double r : probes)
    {
      const std::vector<int> ch = channels_for_ratio(spec.wavenet, r);
      if (std::find(widths.begin(), widths.end(), ch) == widths.end())
      {
        widths.push_back(ch);
        plans.push_back(build_wavenet_plan(slim_wavenet(spec.wavenet, ch), js));
      }
    }
  }
  else if (spec.arch == ARCH_CONTAINER)
    for (const auto& sm : spec.submodels)
      plans.push_back(build_plan(*sm, js));
  else
    plans.push_back(build_plan(spec, js));
  return plans;
}

static void dump_shapes(const char* name, int ft, const WrShapeSet& s)
{
  const std::string h = s.header_text(false), hm = s.header_text(true);
  std::printf("shapes %s ft=%d layers=%zu runs=%zu pairs=%zu heads=%zu posts=%zu programs=%zu header=%zu:%016llx header_masked=%016llx "
              "run_recs=%zu:%016llx\n",
              name, ft, s.layers.size(), s.runs.size(), s.pairs.size(), s.heads.size(), s.posts.size(), s.programs.size(), h.size(),
              wr_hash(h.data(), h.size(), wr_hash_seed), wr_hash(hm.data(), hm.size(), wr_hash_seed), s.run_recs.size(), hash_of(s.run_recs));
  for (size_t i = 0; i < s.programs.size(); i++)
  {
    const WrShapeSet::Program& pr = s.programs[i];
    std::printf("program %s ft=%d p=%zu ops=%zu:%016llx ops_cut=%zu:%016llx split_op=%d,%d,%d,%d first_rec=%d\n", name, ft, i, pr.ops.size(),
                hash_of(pr.ops), pr.ops_cut.size(), hash_of(pr.ops_cut), pr.split_op[0], pr.split_op[1], pr.split_op[2], pr.split_op[3],
                pr.first_rec);
  }
}

int main(int argc, char** argv)
{
  for (int a = 1; a < argc; a++)
  {
    const std::string path = argv[a];
    const size_t slash = path.find_last_of('/');
    const std::string base = slash == std::string::npos ? path : path.substr(slash + 1);
    const char* name = base.c_str();
    for (int ft = 0; ft < 2; ft++)
      for (int shapes = 1; shapes >= 0; shapes--)
        try
        {
          LoadOptions lo;
          lo.fast_tanh = ft != 0;
          const std::shared_ptr<ModelSpec> spec = load_nam_file(path, lo);
          WrShapeSet set;
          const std::vector<Plan> plans = plans_of(*spec, shapes ? &set : nullptr);
          for (size_t i = 0; i < plans.size(); i++)
            dump_plan(name, ft, shapes, i, plans[i]);
          if (shapes)
            dump_shapes(name, ft, set);
        }
        catch (const std::exception& e)
        {
          std::printf("model %s ft=%d shapes=%d error=[%s]\n", name, ft, shapes, one_line(e.what()).c_str());
        }
  }
  std::fflush(stdout);
  return 0;
}
