// module_launch.hpp -- the launch of a module function (a hiprtc instantiation of a run-time struct: rtc.hpp, pencil_launch.hpp), once.
// Host only, the main unit only: nothing here reaches the run-time compiler.
#pragma once
#include <hip/hip_runtime.h>

namespace igx {

// args: the kernel's arguments laid out as its kernarg segment is (natural alignment, in order; zeroed before they are filled in).
// The caller reports a failure its own way.
template <class Args>
static hipError_t module_launch(hipFunction_t fn, unsigned grid, unsigned threads, size_t lds, hipStream_t stream, Args &args) {
  size_t asz = sizeof(Args);
  void *cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &args, HIP_LAUNCH_PARAM_BUFFER_SIZE, &asz, HIP_LAUNCH_PARAM_END};
  return hipModuleLaunchKernel(fn, grid, 1, 1, threads, 1, 1, (unsigned)lds, stream, nullptr, cfg);
}

}  // namespace igx
