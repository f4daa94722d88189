/* scg_jpeg.h — C ABI of libscg_jpg.so: baseline JPEG files packed on the GPU (csrc/jpegpack.hip, gfx950).  The frames of
 * render_video already lie on the device as uint8; here they become complete JPEG files — the frames of a Motion-JPEG video — in
 * three launches per batch, whatever the number of images and their sizes.  The bytes are libjpeg's: Pillow's
 * Image.save(format="JPEG", quality=q, subsampling=s, optimize=False, restart_marker_rows=1) writes the same file.
 *
 * An eighth library next to libscg_raster.so and the six other side libraries.  Its
 * entry points are declared here and in no other header. Conventions as there: plain C, `void* stream` is a hipStream_t (NULL =
 * the default stream), every launch is asynchronous on it, return value 0 = ok, < 0 = invalid argument (the SCG_E_* codes of
 * scg_raster.h), > 0 = a hipError_t; the message of the last failure of the calling thread is scg_jpg_last_error().  Every argument
 * is validated before anything touches a device.  The caller owns all buffers; nothing is allocated, nothing is read back.  No
 * workgroup waits for another; two runs give the same bytes.
 *
 * THE STREAM (the contract: tests/jpeg_refs.py restates it in numpy, Pillow writes the same bytes).
 *
 * Image.  uint8, (H, W, C) contiguous with C = 1 or 3 and 1 <= H, W <= SCG_JPEG_MAX_DIM.  quality 1..100.  C = 3 is R, G, B — or,
 * with bgr, B, G, R read in reverse inside the kernels (no swapped copy exists) — written as Y, Cb, Cr at subsampling
 * SCG_JPEG_444 or SCG_JPEG_420.  C = 1 is a one-component file (subsampling and bgr are ignored).  The file is baseline sequential
 * (SOF0), one interleaved scan, the Huffman tables of T.81 Annex K.3, ONE RESTART INTERVAL PER MCU ROW.
 *
 * Header, in order (lengths and counts big-endian):
 *   SOI    FFD8
 *   APP0   FFE0 0010 "JFIF\0" 01 01 00 0001 0001 00 00
 *   DQT    FFDB 0043 00 + 64 bytes, zigzag order; C = 3: a second one, FFDB 0043 01 + 64 bytes
 *   SOF0   FFC0 0011 08 H W 03 / 01 hv 00 / 02 11 01 / 03 11 01 with hv = 22 (4:2:0) or 11; C = 1: FFC0 000B 08 H W 01 / 01 11 00
 *   DHT    one marker per table: DC0 (00), AC0 (10), and for C = 3 DC1 (01), AC1 (11)
 *   DRI    FFDD 0004 Ri, Ri = MCUs per row — also when the image has a single MCU row
 *   SOS    FFDA 000C 03 01 00 02 11 03 11 00 3F 00; C = 1: FFDA 0008 01 01 00 00 3F 00
 * then the scan, then FFD9.  At most SCG_JPEG_MAX_HEADER bytes.
 *
 * Tables.  s = 5000 / q below q = 50, else 200 - 2 q (integer division); Q[i] = clamp((base[i] * s + 50) / 100, 1, 255) with base the
 * Annex K.1 luminance table (table 0: Y) and chrominance table (table 1: Cb, Cr).
 *
 * Planes, integers throughout.  Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G + 32768 B + 8388608 +
 * 32767) >> 16, Cr = (32768 R - 27439 G - 5329 B + 8388608 + 32767) >> 16; C = 1: Y is the byte.  A full-resolution sample right of
 * or below the image is the last column / row.  At 4:2:0 the chroma sample (cy, cx) is (a + b + c + d + bias) >> 2 with bias 1 for
 * even cx and 2 for odd cx, over the columns min(2 cx, W - 1) and min(2 cx + 1, W - 1) and the rows 2 cy' and min(2 cy' + 1, H - 1),
 * cy' = min(cy, ceil(H / 2) - 1): the rows are padded to an even count, THEN averaged, THEN the last averaged row is repeated
 * (padding the full plane to the MCU height first gives other bytes whenever H % 16 == 8).
 *
 * Blocks.  An MCU is one block per component, at 4:2:0 Y00 Y01 Y10 Y11 Cb Cr.  Y has ceil(W / 8) x ceil(H / 8) real blocks; a
 * luminance block of a 4:2:0 MCU outside them is a DUMMY: all AC zero, DC the quantised DC of the block before it in MCU order
 * (libjpeg's jccoefct.c).  A real block: samples - 128 through libjpeg's jfdctint.c (CONST_BITS 13, PASS1_BITS 2, rows first, the
 * constants 2446 3196 4433 6270 7373 9633 12299 15137 16069 16819 20995 25172, DESCALE(x, n) = (x + (1 << (n - 1))) >> n), then
 * sign(c) * ((|c| + 4 Q) / (8 Q)), an exact integer division.
 *
 * Entropy coding.  Per restart segment (MCU row) the DC predictors start at 0.  T.81 F.1.2: a negative value v is sent as v - 1 in
 * `size` bits, ZRL is F0, EOB 00 only when the block ends in zeros.  Bits MSB first; an FF byte is followed by 00; a segment is
 * padded to a byte with 1-bits and the pad byte is stuffed too; every segment but the image's last is followed by
 * FFD0 + (segment index mod 8).
 *
 * THE CALL.  scg_jpeg_layout gives, for the images' sizes, the image table, the flat SEGMENT table (image, MCU row), the header
 * templates (one per distinct (H, W, C), built here on the host), the default capacities and the workspace; the caller uploads the
 * three tables once per set of shapes and options, only ScgJpegImage.src changes between calls.  scg_jpeg_encode is THREE launches:
 *   count   one workgroup per segment: rounds of SCG_JPEG_THREADS blocks, a block per thread — samples from the pixels, DCT,
 *           quantisation, the quantised coefficients in LDS, the DC chain, the code sizes, a workgroup scan of the bit offsets; the
 *           bits ORed into an LDS window of SCG_JPEG_WINDOW bytes that walks along the segment, only to count bytes and FF bytes;
 *           per segment its stuffed size, the marker behind it included
 *   scan    ONE workgroup: the segments' byte offsets in a fixed-order carry scan (csrc/compact.h); per image what it NEEDS; the
 *           images that fit their capacity back to back, each at a multiple of 16 bytes; the table
 *   encode  one workgroup per segment: the same device functions; the window's bytes written with their stuffing to the segment's
 *           place, then the restart marker or FFD9; an image's first segment also copies the header
 * No per-coefficient workspace exists: the coefficients are formed twice.
 * The table, in the workspace at ScgJpegLayout.table_offset: images + 1 records of four uint32 — (offset, bytes, need, overflow) of
 * every image's file in the output buffer, then (total, images, overflowed images, 0).  An image whose file needs more than
 * ScgJpegImage.capacity has bytes = 0 and overflow = 1, takes no room, and no byte of it is written; `need` is always what the file
 * needs.  The caller reads the table, then exactly `total` bytes.  The bytes between a file's end and the next multiple of 16 are
 * not written.
 */
#ifndef SCG_JPEG_H
#define SCG_JPEG_H

#include "../scg_raster.h"

#define SCG_JPG_ABI_VERSION 1
#define SCG_JPEG_THREADS 256          /* threads of a workgroup in all three kernels: blocks per round */
#define SCG_JPEG_WINDOW 16384         /* bytes of the LDS window of a segment's bits */
#define SCG_JPEG_MAX_DIM 65535        /* H and W */
#define SCG_JPEG_MAX_IMAGES 1048576   /* of one batch */
#define SCG_JPEG_MAX_HEADER 700       /* bytes of a header template (629 with three components, 334 with one) */
#define SCG_JPEG_ALIGN 16             /* every image's file starts at a multiple of it */
#define SCG_JPEG_444 0                /* subsampling, Pillow's numbers */
#define SCG_JPEG_420 2

#ifdef __cplusplus
extern "C" {
#endif

SCG_API const char* scg_jpg_last_error(void);
SCG_API int32_t scg_jpg_abi_version(void);
SCG_API size_t scg_jpg_struct_bytes(int32_t which);     /* sizeof in the library: 0 ScgJpegLayout, 1 ScgJpegImage, 2 ScgJpegSegment,
                                                           3 ScgJpegEncode; else 0 */

/* Offsets into the workspace are multiples of 16.  base: segments + 1 uint32 — the count kernel leaves every segment's stuffed
 * size, the scan kernel turns them into exclusive byte offsets over the flat segment list and their sum; scan: one uint32 per
 * image, the scan kernel's own; table: see above. */
typedef struct ScgJpegLayout {
    uint64_t images, segments;
    uint64_t headers_bytes;           /* of all header templates */
    uint64_t capacity;                /* bytes of the output buffer: sum over the images of their capacity rounded up to 16 */
    uint64_t workspace_bytes;
    uint64_t base_offset, scan_offset;
    uint64_t table_offset, table_bytes;
} ScgJpegLayout;

typedef struct ScgJpegImage {
    uint64_t src;                     /* device address of the (H, W, channels) uint8 pixels; 0 in what scg_jpeg_layout writes */
    int32_t H, W, channels;           /* channels: 1 or 3 */
    int32_t first_segment, segments;  /* in the flat segment list: the MCU rows */
    int32_t mcus;                     /* per MCU row */
    int32_t header_offset, header_bytes;  /* the image's template in the header buffer */
    uint32_t capacity;                /* bytes the file may take; scg_jpeg_layout's default is header_bytes + 3 H W */
    int32_t reserved;                 /* 0 */
} ScgJpegImage;

typedef struct ScgJpegSegment {
    int32_t image;                    /* the segment's image */
    int32_t row;                      /* the MCU row within its image */
} ScgJpegSegment;

/* Host only.  hwc: n triples (H, W, channels).  capacities: n values, or NULL for the default.  images_out: n records,
 * segments_out: out->segments records, headers_out: out->headers_bytes bytes, each or NULL (call once with NULL to learn the
 * sizes).  n = 0 gives an empty layout. */
SCG_API int scg_jpeg_layout(int32_t n, const int32_t* hwc, int32_t quality, int32_t subsampling, const uint32_t* capacities,
                            ScgJpegLayout* out, ScgJpegImage* images_out, ScgJpegSegment* segments_out, uint8_t* headers_out);

typedef struct ScgJpegEncode {
    int32_t struct_bytes;             /* sizeof(ScgJpegEncode) of the caller */
    int32_t images;                   /* >= 1 */
    int32_t quality;                  /* 1..100: the one the header templates were built with */
    int32_t subsampling;              /* SCG_JPEG_444 or SCG_JPEG_420 */
    int32_t bgr;                      /* 0 or 1 */
    int32_t reserved;                 /* 0 */
    uint64_t headers_bytes;           /* of headers_dev */
    const ScgJpegImage* images_host;  /* HOST table, validated before anything is launched: what scg_jpeg_layout gives, src set */
    const ScgJpegImage* images_dev;   /* the same records in device memory */
    const ScgJpegSegment* segments_dev;  /* scg_jpeg_layout's segment table in device memory (a record that names no image or row
                                         of the batch is passed over) */
    const uint8_t* headers_dev;       /* scg_jpeg_layout's header templates in device memory */
} ScgJpegEncode;

/* out[0, out_bytes) with out_bytes >= the sum of the images' capacities rounded up to 16, 16-byte aligned;
 * workspace[0, layout.workspace_bytes), 16-byte aligned.  Three launches; no host read: capturable in a graph at fixed shapes. */
SCG_API int scg_jpeg_encode(const ScgJpegEncode* args, void* out, size_t out_bytes, void* workspace, size_t workspace_bytes,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif
