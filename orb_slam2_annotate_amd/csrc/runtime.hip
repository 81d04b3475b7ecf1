// runtime.hip -- process-wide glue every host file uses: the thread's error text behind orbfe::fail / orbfe_last_error, the
// device count and the public raw allocator of pinned host memory.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/orbfe.h"
#include "host_internal.h"

using namespace orbfe;

static thread_local std::string g_err = "";
int orbfe::fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

extern "C" const char* orbfe_last_error(void) { return g_err.c_str(); }
extern "C" int orbfe_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// ---- pinned host memory (what the pipelined host-batch path transfers at PCIe speed) ----
extern "C" int orbfe_host_alloc(void** p, size_t bytes) {
  if (!p) return fail(ORBFE_ERR_INVALID, "host_alloc: NULL argument");
  *p = nullptr;
  HIPCHK(hipHostMalloc(p, bytes ? bytes : 1, hipHostMallocDefault));
  return ORBFE_OK;
}
extern "C" void orbfe_host_free(void* p) {
  if (p) (void)hipHostFree(p);
}
