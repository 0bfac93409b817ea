// The tuning-knob table (options.h) and its C ABI setter.
#include <stdlib.h>
#include <string.h>

#include "options.h"
#include "vlb_common.h"

namespace {
struct OptRow {
  const char* name;      // vlb_gemm_set_option name
  const char* env;       // environment variable, or null
  int dflt, value;
  bool loaded;           // value is valid: the environment was read, or a set came first
};
#define VLB_OPT_ROW(id, name, env, dflt) {name, env, dflt, 0, false},
OptRow g_opt[VLB_OPT_COUNT] = {VLB_OPTIONS(VLB_OPT_ROW)};
#undef VLB_OPT_ROW
}  // namespace

int vlb_opt(VlbOpt o) {
  OptRow& r = g_opt[o];
  if (!r.loaded) {
    const char* v = r.env ? getenv(r.env) : nullptr;
    r.value = v ? atoi(v) : r.dflt;
    r.loaded = true;
  }
  return r.value;
}

bool vlb_opt_set(const char* name, int value) {
  for (OptRow& r : g_opt)
    if (!strcmp(name, r.name)) {
      r.value = value;
      r.loaded = true;
      return true;
    }
  return false;
}

extern "C" int vlb_gemm_set_option(const char* name, int value) {
  VLB_CHECK_ARG(name && value >= 0, "vlb_gemm_set_option: null name / negative value");
  VLB_CHECK_ARG(vlb_opt_set(name, value), "vlb_gemm_set_option: unknown option %s", name);
  return VLB_OK;
}
