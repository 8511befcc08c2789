// What hg_math.h asks of <hip/hip_runtime.h> when a host check compiles it with a plain C++ compiler behind hip_host_shim.h (-I tests/cpp/hip_stub
// in front): the __host__ qualifier as nothing.  Everything else the kernels use comes from the shim and from the check itself.
#pragma once
#define __host__
