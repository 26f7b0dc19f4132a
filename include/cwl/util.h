// cwl/util.h -- error macros of the reference's cwl/include/cwl/util.h:11-34 on top of the C ABI.
#pragma once
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "../fredholm_hip.h"

namespace cwl
{
// process-wide default context used by the buffer and post-process shims (the reference relies on the CUDA primary context)
inline fh_ctx*& default_context()
{
  static fh_ctx* ctx = nullptr;
  return ctx;
}
// a comma list of device indices ("0,1,2,3"; "0,0" puts two members on one GPU): digits only, no empty entry.  Anything else throws, naming `what`
inline std::vector<int> parse_device_list(const std::string& text, const char* what)
{
  std::vector<int> devices;
  std::string entry;
  for (size_t i = 0; i <= text.size(); ++i) {
    if (i < text.size() && text[i] != ',') { entry += text[i]; continue; }
    if (entry.empty() || entry.size() > 4 || entry.find_first_not_of("0123456789") != std::string::npos)
      throw std::runtime_error(std::string(what) + ": \"" + text + "\" is not a comma list of device indices such as 0,1,2,3");
    devices.push_back(std::atoi(entry.c_str()));
    entry.clear();
  }
  return devices;
}
// the process-wide context over `devices`: one entry is exactly fh_ctx_create, more make a group (fh_ctx_create_group) that renders every frame split across them
inline int create_context(const std::vector<int>& devices, fh_ctx** out)
{
  if (devices.size() == 1) return fh_ctx_create(devices[0], out);
  return fh_ctx_create_group(devices.data(), uint32_t(devices.size()), out);
}
// FH_DEVICES names the devices of the process-wide context; unset: device 0
inline int create_default_context(fh_ctx** out)
{
  const char* e = std::getenv("FH_DEVICES");
  if (!e) return fh_ctx_create(0, out);
  return create_context(parse_device_list(e, "FH_DEVICES"), out);
}
inline fh_ctx* require_context()
{
  fh_ctx*& c = default_context();
  if (!c) {
    if (create_default_context(&c) != FH_OK) throw std::runtime_error(std::string("fh_ctx_create: ") + fh_last_error(nullptr));
  }
  return c;
}
inline void check(fh_ctx* ctx, int rc, const char* what)
{
  if (rc != FH_OK) throw std::runtime_error(std::string(what) + ": " + fh_last_error(ctx));
}
}  // namespace cwl
#define CUDA_SYNC_CHECK() ::cwl::check(::cwl::require_context(), fh_sync(::cwl::require_context()), "sync")

// The reference's applications spell two more things from this header's includes (cwl/include/cwl/util.h:7-21 pulls in <cuda_runtime.h>): the macro
// `CUDA_CHECK(call)` and, as its only argument anywhere in app/, `cudaFree(0)` -- CUDA's idiom for "create the primary context"
// (app/rtcamp8.cpp:75, app/controller.cpp:13).  These are APPLICATION-BOUNDARY NAMES for those two call sites, over the C ABI; nothing under
// fredholm_amd/csrc uses them and no other CUDA runtime name is provided.
typedef int cudaError_t;
static const cudaError_t cudaSuccess = FH_OK;
inline const char* cudaGetErrorString(cudaError_t) { return fh_last_error(::cwl::default_context()); }
inline cudaError_t cudaFree(void* device_ptr)
{
  fh_ctx*& c = ::cwl::default_context();
  if (!c) {
    const int rc = ::cwl::create_default_context(&c);  // cudaFree(0): make the process-wide context (throws when FH_DEVICES cannot be parsed)
    if (rc != FH_OK) return rc;
  }
  return device_ptr ? fh_free(c, device_ptr) : FH_OK;
}
#define CUDA_CHECK(call)                                                                                                                    \
  do {                                                                                                                                      \
    cudaError_t fh_error_ = call;                                                                                                           \
    if (fh_error_ != cudaSuccess) {                                                                                                         \
      throw std::runtime_error(std::string("CUDA call (" #call " ) failed with error: '") + cudaGetErrorString(fh_error_) + "' (" __FILE__ ":" + \
                               std::to_string(__LINE__) + ")\n");                                                                           \
    }                                                                                                                                       \
  } while (0)
