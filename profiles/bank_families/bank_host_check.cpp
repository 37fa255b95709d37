// Host side of model banks as an ordinary executable (for a sanitizer build; no device is touched: nam_hip_bank_create is host-only).
// Arguments: sets of .nam files, each introduced by --accept or --refuse. Every set is loaded, handed to nam_hip_bank_create and
// must be accepted (then nam_hip_bank_n_models answers its size, and the bank is freed AFTER its models) or refused.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/nam_hip.h"

static int run_set(bool accept, const std::vector<const char*>& files)
{
  std::vector<nam_hip_model*> models;
  for (const char* f : files)
  {
    nam_hip_model* m = nullptr;
    if (nam_hip_model_load(f, 1, &m) != NAM_HIP_OK)
    {
      std::printf("FAIL load %s: %s\n", f, nam_hip_last_error());
      return 1;
    }
    models.push_back(m);
  }
  nam_hip_bank* bank = nullptr;
  const int rc = nam_hip_bank_create(models.data(), (int)models.size(), &bank);
  for (nam_hip_model* m : models)
    nam_hip_model_free(m);
  int bad = 0;
  if (accept)
  {
    bad = rc != NAM_HIP_OK || nam_hip_bank_n_models(bank) != (int)files.size();
    std::printf("%s accept, %d members%s%s\n", bad ? "FAIL" : "ok  ", bank ? nam_hip_bank_n_models(bank) : -1, rc ? ": " : "",
                rc ? nam_hip_last_error() : "");
  }
  else
  {
    bad = rc != NAM_HIP_ERR_UNSUPPORTED || bank != nullptr;
    std::printf("%s refuse: %s\n", bad ? "FAIL" : "ok  ", rc ? nam_hip_last_error() : "(accepted)");
  }
  nam_hip_bank_free(bank);
  return bad;
}

int main(int argc, char** argv)
{
  int bad = 0, sets = 0;
  for (int i = 1; i < argc;)
  {
    const bool accept = !std::strcmp(argv[i], "--accept");
    if (!accept && std::strcmp(argv[i], "--refuse"))
    {
      std::printf("usage: bank_host_check (--accept|--refuse FILE...)...\n");
      return 2;
    }
    std::vector<const char*> files;
    for (i++; i < argc && std::strncmp(argv[i], "--", 2); i++)
      files.push_back(argv[i]);
    bad += run_set(accept, files);
    sets++;
  }
  bad += nam_hip_bank_n_models(nullptr) != NAM_HIP_ERR_INVALID_ARGUMENT;
  nam_hip_bank_free(nullptr);
  std::printf("%d sets, %d failed\n", sets, bad);
  return bad ? 1 : 0;
}
