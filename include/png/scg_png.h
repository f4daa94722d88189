/* scg_png.h — C ABI of libscg_png.so: PNG files packed on the GPU (csrc/pngpack.hip, gfx950).  The result images of render_set,
 * render_video and the init stage's snapshot already lie on the device as uint8; here they become the bytes of their files'
 * zlib streams in three launches per batch, whatever the number of images and their sizes.
 *
 * A seventh library next to libscg_raster.so, libscg_io.so, libscg_img.so, libscg_mp.so, libscg_vw.so and libscg_lp.so: its entry
 * points are declared here and in no other header.  Conventions as there: plain C, `void* stream` is a hipStream_t (NULL = the
 * default stream), every launch is asynchronous on it, return value 0 = ok, < 0 = invalid argument (the SCG_E_* codes of
 * scg_raster.h), > 0 = a hipError_t; the message of the last failure of the calling thread is scg_png_last_error().  Every argument
 * is validated before anything touches a device.  The caller owns all buffers; nothing is allocated, nothing is read back.  No
 * workgroup waits for another; two runs give the same bytes.
 *
 * THE STREAM (the contract: tests/png_refs.py restates it in numpy, zlib.decompress and Pillow decode it).
 *
 * Image and filtered stream.  An image is uint8, (H, W, C) contiguous with C = 1 or 3 and 1 <= H, W <= SCG_PNG_MAX_DIM.  C = 3
 * gives colour type 2, bit depth 8, no interlace, bpp = 3.  C = 1 gives colour type 0, bpp = 1 — or, with gray_as_rgb, colour
 * type 2 and bpp = 3 with the byte repeated three times inside the kernels (no expanded copy exists).  The filtered stream has
 * S = H * (1 + W * bpp) bytes, S < 2^31: per row one filter-type byte, then the filtered bytes.  ONE filter per image out of
 * {0 None, 1 Sub, 2 Up, 4 Paeth}, as the PNG specification defines them: a missing neighbour is 0, arithmetic is modulo 256, Paeth
 * ties go left, up, upper-left.
 *
 * Chunks.  SCG_PNG_CHUNK = 32768 bytes of the stream, the last chunk of an image shorter.  A chunk is one deflate block and nothing
 * refers across a chunk border.
 *
 * Tokens.  The chunk is cut into maximal runs of equal bytes.  A run of n < 4 bytes is n literals.  A run of n >= 4: its first byte
 * is a literal; with m = n - 1, m / 258 matches of length 258 at distance 1; then, with r = m % 258, one match of length r when
 * r >= 3, else r literals.  A token is a function of its position, the run's start and the run's length; no search, no other distance.
 *
 * Codes.  Literal/length alphabet of 286 symbols; frequencies from the tokens plus 1 for end-of-block (so at least two are used).
 *   1. the used symbols sorted by (frequency, symbol) ascending
 *   2. the two-queue Huffman merge over that order: leaves in one queue, merged nodes in creation order in the other; the smaller
 *      weight each time, the leaf on a tie
 *   3. the leaves counted per depth
 *   4. the counts above depth 15 added to the count at 15; then, until the Kraft sum (sum of count[l] * 2^(15 - l)) is 2^15:
 *      decrement the count at 15, move one code from the deepest non-empty length below 15 one level down (count[l] -= 1,
 *      count[l + 1] += 2) — miniz's repair
 *   5. lengths from the counts: the most frequent symbols get the shortest lengths (walk the sorted order from its end while the
 *      lengths rise from 1)
 * Codes are canonical (RFC 1951 3.2.2).  The distance alphabet is declared with two codes of length 1; every match uses distance
 * symbol 0: one bit, no extra bits.
 *
 * Block.  BFINAL = 1 only in the image's last chunk; BTYPE = 10; HLIT = 29, HDIST = 1, HCLEN = 15; the 19 three-bit lengths of the
 * code-length code in RFC order: 4 for the symbols 0..15, 0 for 16, 17, 18; then 288 code lengths (286 literal/length, 2 distance),
 * 4 bits each, no run symbols: SCG_PNG_HEADER_BITS = 1226 bits for every block.  Then the tokens and end-of-block.  A non-final
 * block is followed by an empty stored block (bits 000, zero padding to a byte, 00 00 FF FF), so every chunk starts on a byte; the
 * final block is zero-padded to a byte.  If the block's bytes, that tail included, are >= n + 5 for a chunk of n bytes, a stored
 * block is emitted instead: BFINAL, LEN, ~LEN, the n filtered bytes.  No chunk expands by more than 5 bytes.
 *
 * Zlib stream: 78 01, the blocks, the big-endian Adler-32 of the filtered stream (from per-chunk partial sums, exact integers modulo
 * 65521).  The FILE — signature, IHDR, ONE IDAT, IEND — is the host's: its 41 leading bytes, the IDAT's CRC-32 and IEND are not
 * written here.
 *
 * THE CALL.  scg_png_layout gives, for the images' sizes, the image table and the chunk table (the caller uploads both once per set
 * of shapes; only ScgPngImage.src changes between calls), the capacity of the output buffer — 16 * images + sum over the images of
 * (S + 5 * chunks + 6) — and the workspace.  scg_png_encode is THREE launches:
 *   count   one workgroup per chunk of the flat chunk list: the filtered bytes in LDS, run starts, token roles, the 286-bin
 *           histogram, the Adler partial sums, the code (a bitonic sort of 512 keys, the serial merge by one lane); per chunk the
 *           288 lengths, the block's kind and byte size, the partial sums
 *   scan    ONE workgroup: the chunks' byte offsets in a fixed-order carry scan (csrc/compact.h); the images' streams back to
 *           back, each starting at a multiple of 16 bytes; per image its 78 01 and its Adler-32; the table
 *   encode  one workgroup per chunk: the same filtered bytes and tokens by the same device functions, the canonical codes, a
 *           workgroup-exclusive scan of the lanes' bit counts, the bits ORed into a zeroed LDS image, the block written to its byte
 *           offset — edges as bytes, the middle as dwords, never a byte of a neighbour's
 * The table, in the workspace at ScgPngLayout.table_offset: images + 1 pairs of uint32 — (offset, bytes) of every image's zlib
 * stream in the output buffer, then (total, images): the caller reads the table, then exactly `total` bytes.  The bytes between a
 * stream's end and the next multiple of 16 are not written.
 */
#ifndef SCG_PNG_H
#define SCG_PNG_H

#include "../scg_raster.h"

#define SCG_PNG_ABI_VERSION 1
#define SCG_PNG_CHUNK 32768           /* bytes of the filtered stream per deflate block */
#define SCG_PNG_THREADS 256           /* threads of a workgroup in all three kernels */
#define SCG_PNG_SYMBOLS 286           /* literal/length alphabet */
#define SCG_PNG_LENGTHS 288           /* code lengths of a block's header: 286 literal/length, 2 distance */
#define SCG_PNG_HEADER_BITS 1226      /* of every dynamic block */
#define SCG_PNG_MAX_CODE_BITS 15
#define SCG_PNG_MAX_DIM 65535         /* H and W */
#define SCG_PNG_MAX_STREAM 2147483647 /* S < 2^31 */
#define SCG_PNG_MAX_IMAGES 1048576    /* of one batch */
#define SCG_PNG_ALIGN 16              /* every image's stream starts at a multiple of it */
#define SCG_PNG_FILTER_NONE 0
#define SCG_PNG_FILTER_SUB 1
#define SCG_PNG_FILTER_UP 2
#define SCG_PNG_FILTER_PAETH 4
#define SCG_PNG_KIND_DYNAMIC 0        /* ScgPngChunkInfo.kind */
#define SCG_PNG_KIND_STORED 1

#ifdef __cplusplus
extern "C" {
#endif

SCG_API const char* scg_png_last_error(void);
SCG_API int32_t scg_png_abi_version(void);
SCG_API size_t scg_png_struct_bytes(int32_t which);     /* sizeof in the library: 0 ScgPngLayout, 1 ScgPngImage, 2 ScgPngChunk,
                                                           3 ScgPngChunkInfo, 4 ScgPngEncode; else 0 */

/* Offsets into the workspace are multiples of 16.  lengths: SCG_PNG_LENGTHS bytes per chunk; info: one ScgPngChunkInfo per chunk;
 * base: chunks + 1 uint32, the exclusive byte offsets of the blocks over the flat chunk list and their sum; scan: one uint32 per
 * image, the scan kernel's own; table: see above. */
typedef struct ScgPngLayout {
    uint64_t images, chunks;
    uint64_t capacity;                /* bytes of the output buffer: 16 * images + sum(S + 5 * chunks + 6) */
    uint64_t workspace_bytes;
    uint64_t lengths_offset, info_offset, base_offset, scan_offset;
    uint64_t table_offset, table_bytes;
} ScgPngLayout;

typedef struct ScgPngImage {
    uint64_t src;                     /* device address of the (H, W, channels) uint8 pixels; 0 in what scg_png_layout writes */
    int32_t H, W, channels;           /* channels: 1 or 3 */
    int32_t first_chunk, chunks;      /* in the flat chunk list */
    int32_t stream_bytes;             /* S */
} ScgPngImage;

typedef struct ScgPngChunk {
    int32_t image;                    /* the chunk's image */
    int32_t index;                    /* the chunk within its image: stream bytes [index * SCG_PNG_CHUNK, ...) */
} ScgPngChunk;

typedef struct ScgPngChunkInfo {      /* what the count kernel leaves per chunk */
    uint32_t bytes;                   /* of the block, its tail included */
    uint32_t kind;                    /* SCG_PNG_KIND_* */
    uint32_t sum_a, sum_b;            /* sum of d[i] and sum of (n - i) * d[i] over the chunk's n bytes, each modulo 65521 */
} ScgPngChunkInfo;

/* Host only.  hwc: n triples (H, W, channels).  images_out: n records, chunks_out: out->chunks records, or NULL (call once with
 * NULL to learn `chunks`).  n = 0 gives an empty layout. */
SCG_API int scg_png_layout(int32_t n, const int32_t* hwc, int32_t gray_as_rgb, ScgPngLayout* out, ScgPngImage* images_out,
                           ScgPngChunk* chunks_out);

typedef struct ScgPngEncode {
    int32_t struct_bytes;             /* sizeof(ScgPngEncode) of the caller */
    int32_t images;                   /* >= 1 */
    int32_t filter;                   /* SCG_PNG_FILTER_* */
    int32_t gray_as_rgb;              /* 0 or 1 */
    const ScgPngImage* images_host;   /* HOST table, validated before anything is launched: what scg_png_layout gives, src set */
    const ScgPngImage* images_dev;    /* the same records in device memory */
    const ScgPngChunk* chunks_dev;    /* scg_png_layout's chunk table in device memory (a record that names no image or chunk of
                                         the batch, or a block that would end behind the capacity, is passed over) */
} ScgPngEncode;

/* out[0, layout.capacity), 16-byte aligned; workspace[0, layout.workspace_bytes), 16-byte aligned.  Three launches; no host read:
 * capturable in a graph at fixed shapes. */
SCG_API int scg_png_encode(const ScgPngEncode* args, void* out, size_t out_bytes, void* workspace, size_t workspace_bytes,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif
