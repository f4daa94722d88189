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

    // the buffers of a batch entry point `who` (scg_png_encode, scg_jpeg_encode), behind the checks of its own arguments: the
    // output against the layout's capacity, the workspace against the layout's need, then the two device tables' alignment
    int check_batch_buffers(const char* who, const void* out, size_t out_bytes, uint64_t capacity, const void* workspace,
                            size_t workspace_bytes, uint64_t needed, const void* table_a, size_t align_a, const void* table_b,
                            size_t align_b) {
        if (!out) return fail(SCG_E_NULL, "%s: out is NULL", who);
        if (out_bytes < capacity) return fail(SCG_E_SCRATCH, "%s: out of %zu bytes < %llu", who, out_bytes, (unsigned long long)capacity);
        if (reinterpret_cast<uintptr_t>(out) % 16) return fail(SCG_E_ALIGN, "%s: out not 16-byte aligned", who);
        if (!workspace) return fail(SCG_E_NULL, "%s: workspace is NULL", who);
        if (workspace_bytes < needed)
            return fail(SCG_E_SCRATCH, "%s: workspace of %zu bytes < %llu", who, workspace_bytes, (unsigned long long)needed);
        if (reinterpret_cast<uintptr_t>(workspace) % 16) return fail(SCG_E_ALIGN, "%s: workspace not 16-byte aligned", who);
        if (reinterpret_cast<uintptr_t>(table_a) % align_a || reinterpret_cast<uintptr_t>(table_b) % align_b)
            return fail(SCG_E_ALIGN, "%s: a device table is not aligned to its records", who);
        return 0;
    }
};

}  // namespace scg
