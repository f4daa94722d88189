// host_error.h — the error text of one library, host side only.  Every library (libscg_raster.so and each of the side libraries)
// owns exactly one `thread_local ErrorText` and returns its `text` from its *_last_error(): no library reads another's.
// A plain aggregate without a constructor: a thread_local object of it is constant-initialised to the empty string, as a bare
// `thread_local char[512] = ""` is.
#pragma once

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/scg_raster.h"

namespace scg {

struct ErrorText {
    char text[512];

    int vfail(int code, const char* fmt, va_list ap) {
        vsnprintf(text, sizeof(text), fmt, ap);
        return code;
    }

    int fail(int code, const char* fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        vfail(code, fmt, ap);
        va_end(ap);
        return code;
    }

    int check_hip(hipError_t e, const char* what) {
        if (e == hipSuccess) return 0;
        snprintf(text, sizeof(text), "%s: %s (hipError %d)", what, hipGetErrorString(e), (int)e);
        return (int)e;
    }

    // a required pointer of entry point `who`: NULL, then misaligned
    int check_ptr(const char* who, const void* p, const char* name, size_t align) {
        if (!p) return fail(SCG_E_NULL, "%s: %s is NULL", who, name);
        if (reinterpret_cast<uintptr_t>(p) % align) return fail(SCG_E_ALIGN, "%s: %s is not %zu-byte aligned", who, name, align);
        return 0;
    }
};

}  // namespace scg
