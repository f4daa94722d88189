/* scg_ply.h — C ABI of libscg_io.so: the bodies of the reference's scene files (scene/gaussian_model.py:565-609 save_ply,
 * :653-756 load_ply; scene/dataset_readers.py:127-142 storePly) packed and unpacked on the GPU (csrc/plypack.hip, gfx950).
 *
 * A second library next to libscg_raster.so: its entry points are declared here and in no header directly under include/.  Conventions as
 * there: plain C, `void* stream` is a hipStream_t (NULL = the default stream), every launch is asynchronous on it, return value
 * 0 = ok, < 0 = invalid argument (the SCG_E_* codes of scg_raster.h), > 0 = a hipError_t; the message of the last failure of the
 * calling thread is scg_io_last_error().  Arguments are validated before anything touches a device.
 *
 * The files (all binary little-endian PLY, one `vertex` element):
 *   point_cloud.ply        69 floats per ray-bound Gaussian: x y z (= rayo + rayd * zval, the product and the sum rounded one after
 *                          the other) nx ny nz (0) | f_dc_0..2 | f_rest_0..44 (file column c * 15 + j = memory element (j, c)) |
 *                          opacity | scale_0..2 | rot_0..3 | zval_0 | rayo_0..2 | rayd_0..2
 *   point_cloud_bg.ply     62 floats per background Gaussian: bx by bz bnx bny bnz | bf_dc | bf_rest | bopacity | bscale | brot
 *   point_cloud_color.ply  27 bytes per Gaussian, the ray-bound rows first: x y z nx ny nz (float) red green blue (uchar)
 * Whatever is not computed is copied bit for bit (NaN payloads, signs of zero and denormals arrive unchanged).
 *
 * The colour byte B(v) of a float v is what numpy's array cast to uint8 gives on x86-64: for a finite |v| < 2^31 the low 8 bits
 * of the two's-complement int32 of trunc(v) (-1 -> 255, 256 -> 0); 0 for every other v (|v| >= 2^31, the infinities, NaN).
 */
#ifndef SCG_PLY_H
#define SCG_PLY_H

#include "../scg_raster.h"

#define SCG_IO_ABI_VERSION 1
#define SCG_PLY_TILE_ROWS 64        /* rows (records) one workgroup stages through LDS; a multiple of 4, so a tile of 27-byte
                                       records is a whole number of dwords */
#define SCG_PLY_RAY_FLOATS 69       /* dwords of a point_cloud.ply record = destination columns of its unpack table */
#define SCG_PLY_BG_FLOATS 62        /* ... of a point_cloud_bg.ply record */
#define SCG_PLY_COLOR_BYTES 27      /* bytes of a point_cloud_color.ply record */
#define SCG_PLY_MAX_STRIDE 224      /* dwords of the widest record scg_ply_unpack stages (extra properties included) */

#ifdef __cplusplus
extern "C" {
#endif

SCG_API const char* scg_io_last_error(void);
SCG_API int32_t scg_io_abi_version(void);

/* Byte offsets (each a multiple of 256) and sizes of the three bodies in the ONE buffer scg_ply_pack writes.  color_bytes is
 * (nr + nb) * 27 rounded up to a multiple of 4: the padding is zero and is never written to a file. */
typedef struct ScgPlyLayout {
    uint64_t ray_offset, ray_bytes;
    uint64_t bg_offset, bg_bytes;
    uint64_t color_offset, color_bytes;
    uint64_t total;
} ScgPlyLayout;
SCG_API size_t scg_ply_layout_bytes(void);      /* sizeof(ScgPlyLayout) in the library */
SCG_API int scg_ply_layout(int32_t nr, int32_t nb, ScgPlyLayout* out);

/* The three bodies of `model` (nr = model->ray.count, nb = model->bg.count) into buffer[0, layout.total), 16-byte aligned.  One
 * launch; nothing is launched when both counts are 0. */
SCG_API int scg_ply_pack(const ScgModel* model, void* buffer, size_t buffer_bytes, void* stream);

/* The colour file alone with the VIEW-DEPENDENT colour of gaussian_renderer/__init__.py:89-96:
 *   B(max(eval_sh(sh_degree, sh, dir) + 0.5, 0) * 255),  dir = (xyz - campos) / sqrt((dx * dx + dy * dy) + dz * dz)
 * every operation rounded on its own, the polynomial the rasterizer's (csrc/sh_eval.h).  campos: 3 floats on the device.
 * buffer: ((nr + nb) * 27 rounded up to 4) bytes, 16-byte aligned.  One launch. */
SCG_API int scg_ply_pack_color_view(const ScgModel* model, int32_t sh_degree, const float* campos, void* buffer,
                                    size_t buffer_bytes, void* stream);

/* The inverse of the ray-bound body (bg = 0) or of the background body (bg = 1).  `upload` holds `rows` records of `stride`
 * dwords (body_bytes = rows * stride * 4) and, right behind them, a table of 69 (bg: 62) int32: table[d] = the dword of the
 * record that destination column d — the column order of this library's own files, above — is read from.  Columns nothing is
 * loaded from (x y z nx ny nz of a ray-bound file, bnx bny bnz) are ignored but must still lie inside the record.  The table is
 * validated on `table_host`, while the kernel reads the copy behind the body: THE CALLER GUARANTEES that the two hold the same
 * values (the kernel clamps the entries of its copy into the record and checks nothing else: a copy that differs loads other columns).  The tensors of model->ray (bg: model->bg; count =
 * rows) are WRITTEN: features_rest with the inverse transposition, everything as a bit copy.  One launch. */
SCG_API int scg_ply_unpack(const void* upload, size_t body_bytes, const int32_t* table_host, int32_t rows, int32_t stride,
                           int32_t bg, const ScgModel* model, void* stream);

#ifdef __cplusplus
}
#endif
#endif
