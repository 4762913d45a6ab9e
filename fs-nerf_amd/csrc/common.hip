// common.hip — thread-local error string, version, device query, the debug build's record registry.
#include "common.hpp"

#include <cstring>
#include <mutex>
#include <string>
#include <vector>

namespace fsn {
static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int hip_fail(hipError_t e, const char* what) {
  set_error("HIP error %d (%s) at %s", (int)e, hipGetErrorString(e), what);
  return FSN_E_HIP;
}
}  // namespace fsn

extern "C" int fsn_version(void) { return 100; }
extern "C" const char* fsn_last_error(void) { return fsn::g_err; }

#ifdef FSN_DEBUG
namespace fsn {
namespace {
struct DebugUnit {
  const char* name;
  debug_take_fn take;
};
// function-local: the registrars of other translation units may run before this file's own static initialisers
std::vector<DebugUnit>& debug_units() {
  static std::vector<DebugUnit> units;
  return units;
}
}  // namespace

void debug_register(const char* unit, debug_take_fn take) {  // kept sorted by name: link order does not show
  auto& units = debug_units();
  auto at = units.begin();
  while (at != units.end() && strcmp(at->name, unit) < 0) ++at;
  units.insert(at, DebugUnit{unit, take});
}
}  // namespace fsn
#endif

extern "C" const char* fsn_debug_units(void) {
#ifdef FSN_DEBUG
  static const std::string names = [] {
    std::string s;
    for (const auto& u : fsn::debug_units()) s += (s.empty() ? "" : ",") + std::string(u.name);
    return s;
  }();
  return names.c_str();
#else
  return "";
#endif
}

extern "C" int fsn_debug_report(const char* unit, uint32_t* out4) {
  FSN_REQUIRE(unit && out4, FSN_E_INVALID, "fsn_debug_report: null pointer");
#ifdef FSN_DEBUG
  for (const auto& u : fsn::debug_units()) {
    if (strcmp(u.name, unit) != 0) continue;
    FSN_HIP(hipDeviceSynchronize());
    return u.take(out4);
  }
  FSN_REQUIRE(false, FSN_E_INVALID, "fsn_debug_report: no unit '%s' (units: %s)", unit, fsn_debug_units());
#else
  FSN_REQUIRE(false, FSN_E_UNSUPPORTED, "fsn_debug_report: not a debug build (make -C fs-nerf_amd/csrc debug)");
#endif
}

extern "C" int fsn_device_cus(void) {
  int dev = 0;
  FSN_HIP(hipGetDevice(&dev));
  int cus = 0;
  FSN_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  return cus;
}
