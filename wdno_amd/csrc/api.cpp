// api.cpp -- library-level entry points of libwdno_hip (error strings, version).
#include <hip/hip_runtime.h>
#include "common.h"
#include "debug_modes.h"

thread_local hipError_t wdno_tls_last_hip_error = hipSuccess;

extern "C" const char* wdno_strerror(int code) {
  switch (code) {
    case WDNO_OK: return "ok";
    case WDNO_EINVAL: return "invalid argument";
    case WDNO_ELAUNCH: return "kernel launch failed";
    case WDNO_EUNSUPPORTED: return "unsupported configuration";
    case WDNO_EWORKSPACE: return "workspace too small";
    default: return "unknown error";
  }
}
extern "C" int wdno_version(void) { return 100; }
extern "C" const char* wdno_last_hip_error(void) { return hipGetErrorString(wdno_tls_last_hip_error); }

int wdno_num_cus() {
  static int n = 0;
  if (!n) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 256;
    n = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }
  return n;
}

// kernel-selection switches for A/B measurements and tests (debug_modes.h is the list); 0 in production
int wdno_debug_mode = WDNO_DBG_OFF;
extern "C" int wdno_set_debug(int mode) {
  switch (mode) {
#define WDNO_DBG_CASE(name, value) case name:
    WDNO_DEBUG_MODES(WDNO_DBG_CASE)
#undef WDNO_DBG_CASE
      wdno_debug_mode = mode;
      return WDNO_OK;
    default: return WDNO_EINVAL;
  }
}
