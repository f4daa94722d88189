/* scg_resample.h — C ABI of libscg_img.so: the camera images' downsizing on the GPU (csrc/resample.hip, gfx950).
 *
 * The reference resizes every image in loadCam (utils/camera_utils.py:44) with PILtoTorch (utils/general_utils.py:22-28):
 * Pillow's Image.resize(size) with its default filter, bicubic, then / 255.0.  For 8-bit images that resampler is integer
 * arithmetic, so the kernels equal it byte for byte.
 *
 * A third library next to libscg_raster.so and libscg_io.so: its entry points are declared here and in no other header.
 * Conventions as there: plain C, `void* stream` is a hipStream_t (NULL = the default stream), every launch is asynchronous on it,
 * return value 0 = ok, < 0 = invalid argument (the SCG_E_* codes of scg_raster.h), > 0 = a hipError_t; the message of the last
 * failure of the calling thread is scg_img_last_error().  Arguments are validated before anything touches a device.  The caller owns
 * every buffer, the intermediate included; nothing is allocated, nothing is read by the host, nothing is atomic.
 *
 * The rule, per axis (inS -> outS), each axis on its own, the horizontal one first and rounded to bytes:
 *   tables (built by the caller in IEEE double, scgaussian_amd/images.py axis_table): for output index i a window
 *   bounds[2 i] = first source index, bounds[2 i + 1] = count, and coeffs[i * ksize + 0 .. count) = the bicubic weights (a = -0.5,
 *   support 2 * max(inS / outS, 1)), normalised and rounded to 22 fractional bits;
 *   a pass: acc = 2^21 + sum(src[first + t] * coeffs[t]) in int32, out = clamp(acc >> 22, 0, 255), the shift arithmetic.
 * An axis whose size does not change is not resampled: its tables are NULL.
 * The float image is float(byte) / 255.0f, the division correctly rounded, laid out (C, H, W).
 */
#ifndef SCG_RESAMPLE_H
#define SCG_RESAMPLE_H

#include "../scg_raster.h"

#define SCG_IMG_ABI_VERSION 1
#define SCG_RESAMPLE_MAX_KSIZE 129      /* coefficients per output sample: a 32x downscale; beyond it the caller resizes on the host */
#define SCG_RESAMPLE_MAX_SIZE 65535     /* widths, heights and images per call */
#define SCG_RESAMPLE_STRIP 32           /* output columns one workgroup of the horizontal pass owns */
#define SCG_RESAMPLE_STRIP_ROWS 32      /* ... over this many source rows */
#define SCG_RESAMPLE_VTILE 1024         /* output bytes of a row one workgroup of the vertical pass owns (4 per thread) */
#define SCG_RESAMPLE_PITCH_ALIGN 16     /* the intermediate's row pitch is a multiple of this many bytes */

#ifdef __cplusplus
extern "C" {
#endif

SCG_API const char* scg_img_last_error(void);
SCG_API int32_t scg_img_abi_version(void);

/* Bytes of one row of the intermediate: wout * channels rounded up to SCG_RESAMPLE_PITCH_ALIGN; 0 for arguments out of range. */
SCG_API size_t scg_resample_pitch(int32_t wout, int32_t channels);

/* Bytes of the intermediate of scg_resample_u8: n * hin * pitch when the width changes, otherwise 0; 0 for arguments out of range. */
SCG_API size_t scg_resample_mid_bytes(int32_t n, int32_t hin, int32_t win, int32_t channels, int32_t wout);

/* `n` tightly packed uint8 images (hin, win, channels), one behind the other from `src`, to (hout, wout, channels) in `out`
 * and, when out_float is not NULL, to float (channels, hout, wout) per image in `out_float`.  channels is 1 or 3.
 *
 * src may start at any byte address: the horizontal pass reads the aligned dwords that hold its bytes (a device allocation is a
 * whole number of dwords).  hbounds (wout * 2 int32) / hcoeffs (wout * hksize int32) are the width's tables, required when
 * wout != win and ignored otherwise, and vbounds / vcoeffs (hout * 2, hout * vksize) the height's, required when hout != hin; all
 * on the device.  THE CALLER GUARANTEES that they are the tables of these sizes: the kernels clamp every window into the source and
 * into its ksize coefficients and check nothing else (other tables give other bytes, never an access outside a buffer).
 * mid: the intermediate (n, hin, pitch) of scg_resample_mid_bytes bytes, SCG_RESAMPLE_PITCH_ALIGN-byte aligned; ignored (may be
 * NULL) when wout == win.  out: n * hout * wout * channels bytes; out_float: 4 times as many, 4-byte aligned.
 *
 * At most two launches: the horizontal pass (only when wout != win) src -> mid, then the vertical pass, which also writes the
 * tight output and the float image; when hout == hin it copies. */
SCG_API int scg_resample_u8(const uint8_t* src, int32_t n, int32_t hin, int32_t win, int32_t channels, int32_t hout, int32_t wout,
                            const int32_t* hbounds, const int32_t* hcoeffs, int32_t hksize,
                            const int32_t* vbounds, const int32_t* vcoeffs, int32_t vksize,
                            void* mid, size_t mid_bytes, uint8_t* out, size_t out_bytes, float* out_float, size_t out_float_bytes,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif
