// The error text of a C entry point, said once (host only).  A translation unit names the buffer its header's *_last_error returns
//     #define EX4D_ERROR_BUFFER ex4d_loss_error_buffer        (ex4d_loss.hip)   or   ex4d_densify_error_buffer   (ex4d_densify.hip)
// before including this file, and its entry points read: clear_error(); refuse with `return fail(status, text);`; launch;
// `return launch_status("name");`.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdio>
#include "../../include/ex4d_rasterizer.h"      // the status codes

#ifndef EX4D_ERROR_BUFFER
#error "define EX4D_ERROR_BUFFER to the accessor of the error text before including ex4d_host_error.h"
#endif
char *EX4D_ERROR_BUFFER(size_t *capacity);

namespace {

int fail(int status, const char *text)
{
    size_t cap = 0;
    char *buf = EX4D_ERROR_BUFFER(&cap);
    snprintf(buf, cap, "%s", text);
    return status;
}

void clear_error()
{
    size_t cap = 0;
    EX4D_ERROR_BUFFER(&cap)[0] = 0;
}

int launch_status(const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return EX4D_OK;
    size_t cap = 0;
    char *buf = EX4D_ERROR_BUFFER(&cap);
    snprintf(buf, cap, "%s: launch failed: %s", what, hipGetErrorString(e));
    return EX4D_ERR_HIP;
}

}  // namespace
