/* scg_jpegdec.h — C ABI of libscg_jpegdec.so: baseline JPEG files decoded on the GPU (csrc/jpegunpack.hip, gfx950).  The reading
 * direction of include/jpg/scg_jpeg.h: the file's bytes are uploaded, the tight uint8 (H, W, 3) or (H, W) pixels appear on the
 * device, the pixels np.asarray(Image.open(path)) gives (Pillow on libjpeg-turbo), byte for byte.
 *
 * A side library (build.SIDE_LIBRARIES "jpegdec").  Conventions as in the other libraries: plain C, pointers and scalars only, `void* stream`
 * is a hipStream_t (NULL = the default stream), every launch is asynchronous on it, return value 0 = ok, < 0 = invalid argument
 * (the SCG_E_* codes of scg_raster.h), > 0 = a hipError_t; the message of the last failure of the calling thread is
 * scg_jpegdec_last_error().  Every argument is validated before anything touches a device.  The caller owns all buffers: nothing
 * is allocated, nothing is read back, no float atomics; two runs give the same bytes.
 *
 * WHAT IS ACCEPTED (the caller's parser refuses everything else and decodes it on the host):
 *   baseline sequential (SOF0), 8-bit precision; ONE interleaved scan with every component, Ss = 0, Se = 63, Ah = Al = 0; Huffman
 *   coding with any DHT tables (ids 0 and 1 of each class; the all-ones code word reserved, as T.81 demands); 8-bit DQT (Pq = 0);
 *   one component, or three as Y Cb Cr with sampling 1x1, 2x1 or 2x2 on Y and 1x1 on Cb and Cr; DRI / RSTn at any interval or none.
 *
 * THE RULE (tests/jpegdec_refs.py restates it in numpy).
 *
 * Entropy decoding: T.81 F.2.2.  `FF 00` stands for one FF byte.  At RSTn the reader skips to the byte after the marker, sets the
 * DC predictors to 0 and starts a new MCU.  DC sizes 0..11 and AC sizes 1..10 are taken; a code no table holds, a larger size, a
 * zigzag index beyond 63, a restart marker that is not where and what the interval says, and a block count other than the
 * frame's are REPORTED (the status word), never repaired.
 * Dequantisation: coefficient * table entry in int32.
 * Inverse DCT: libjpeg's jidctint "islow": 13-bit constants FIX(x) = round(x * 8192) (2446 3196 4433 6270 7373 9633 12299 15137
 * 16069 16819 20995 25172), PASS1_BITS = 2; columns first with a rounded shift by 11, then rows with a rounded shift by 18, then
 * + 128 and a clamp to 0..255.  Rounded shifts are arithmetic: (x + (1 << (s - 1))) >> s.  Outside the range a real encoder can
 * produce libjpeg's C range table WRAPS and its SIMD code SATURATES; the kernel saturates, and equality with Pillow is claimed
 * only where those two agree.
 * Chroma planes: a subsampled plane is cropped to ceil(W / 2) columns (2x1, 2x2) and ceil(H / 2) rows (2x2) BEFORE upsampling; a
 * neighbour beyond an edge is the edge sample itself.  The padding columns and rows of the last MCU never reach a pixel.
 * 2x1 ("fancy" h2v1): out[2i] = (3 c[i] + c[i-1] + 1) >> 2, out[2i+1] = (3 c[i] + c[i+1] + 2) >> 2; the first and the last output
 * sample are the first and last input sample unchanged (a plane of one column is duplicated).
 * 2x2 ("fancy" h2v2): per output row s[i] = 3 near[i] + far[i], far the row above for even output rows and the row below for odd
 * ones; out[2i] = (3 s[i] + s[i-1] + 8) >> 4, out[2i+1] = (3 s[i] + s[i+1] + 7) >> 4; at the two ends the missing neighbour is
 * s[i] itself.
 * Colour: R = Y + ((91881 (Cr-128) + 32768) >> 16), B = Y + ((116130 (Cb-128) + 32768) >> 16),
 * G = Y + ((-22554 (Cb-128) - 46802 (Cr-128) + 32768) >> 16), each clamped.  One component gives the (H, W) plane.
 * EXIF orientation is not applied (Image.open does not apply it either).
 *
 * THE CALL.  The entropy-coded segment is ONE serial bit stream; it is cut into subsequences of SCG_JPEGDEC_SUBSEQ bytes, one
 * thread each, SCG_JPEGDEC_THREADS of them a workgroup.  A decoder state is (bit position in the stuffed stream, block within the
 * MCU, zigzag index); a subsequence's EXIT state is the state at the first symbol (a code word with its value bits) that begins
 * at or beyond its end.
 *   sync    round 0: every thread decodes from (its first bit, 0, 0) and keeps its exit state.  Then a thread whose predecessor's
 *           exit state is not the state it started from decodes again from it: inside a workgroup in LDS behind barriers until
 *           nothing changes (at most SCG_JPEGDEC_THREADS times), across workgroups one launch per round through a double-buffered
 *           word per workgroup.  Subsequence 0 starts from the truth, so every round fixes at least one more; a Huffman stream
 *           resynchronises after a few symbols and a restart marker resets EVERY state, so three launches do in practice.  A round
 *           beyond convergence changes nothing.  Per launch a device word counts the workgroups whose first state changed.
 *   count   from the converged states: the blocks that END in each subsequence, the sums of the DC differences per component
 *           behind the last restart marker in it, whether it held one.
 *   scan    ONE workgroup, fixed order: the first block of every subsequence (csrc/compact.h carry_scan) and its DC predictors
 *           (the same scan under the operator of (reset flag, sum)); the status words.
 *   write   the same decode once more: int16 coefficients in natural order into the coefficient buffer, block after block in
 *           stream order; a block that spans subsequences is continued by each at its own zigzag index.  The buffer is cleared
 *           inside the call.
 *   idct    eight threads a block: dequantise, the columns, the rows; the 8 x 8 transposition through LDS rows of 9 dwords;
 *           8 bytes of a component plane per thread.
 *   colour  crop, upsample, convert: a lane owns 4 output bytes of a row, a dword store where the address is aligned.
 * Every read of the stream is bounded: beyond the segment's end the reader sees no bits and stops, wherever a wrong state led it.
 *
 * The header block (device memory, SCG_JPEGDEC_HEADER_BYTES, little-endian, 16-byte aligned), built by the caller:
 *   [0, 512)       uint16 quant[4][64], natural order, by table id
 *   [512, 4096)    four Huffman tables of 896 bytes: DC id 0, DC id 1, AC id 0, AC id 1; each
 *                  uint16 look[256]   by the next 8 bits: (length << 8) | symbol for a code of at most 8 bits, else 0
 *                  int32 maxcode[16]  the largest code of length l at [l - 1], -1 without one
 *                  int32 valoff[16]   index of the first value of length l minus its first code
 *                  uint8 vals[256]
 * The kernels mask every index they take from it.
 * The frame (HOST memory, SCG_JPEGDEC_FRAME_WORDS int32): H, W, components, h, v (Y's sampling factors), restart interval in
 * MCUs (0: none), quant table id of each of three components, DC table id of each, AC table id of each, 0.
 * The status (the first four uint32 of the workspace; the call's ONE host read): [0] the SCG_JPEGDEC_BAD_* bits, 0 = the pixels are
 * right; [1] sync launches until nothing changed (0: not within those run); [2] blocks counted; [3] 0.
 *
 * THE BATCH.  Nothing in the decode of one file depends on another file, so scg_jpegdec_decode_batch puts n images into the SAME
 * seven steps (two clears, the sync launches, count, scan, write, idct, colour) whatever n is.  The rule above is not restated:
 * the decode, the idct, the upsampling and the colour conversion are the same device functions over an image view (frame and
 * pointers), which the single entry fills from its arguments and the batched kernels from the image table.  A workgroup lies
 * inside ONE image and finds it from its index alone by a search of a prefix table (uniform: scalar loads); thread t of an image's
 * workgroup g owns subsequence g * SCG_JPEGDEC_THREADS + t of THAT image; subsequence 0 of every image starts from the truth; the
 * hand-over words, the change counters and the status are per image, and no state crosses from one image into the next.  The scan
 * runs one workgroup per image.  Idct and colour run flat grids over all images' blocks and (row, chunk of 4 *
 * SCG_JPEGDEC_THREADS bytes) pairs.  Every offset a kernel takes from the DEVICE table is held to the buffer sizes the call was
 * passed: a device table that differs from the host copy gives wrong pixels or a status bit (an image whose record cannot be
 * followed reports SCG_JPEGDEC_BAD_SYNC | SCG_JPEGDEC_BAD_COUNT), never an access outside a buffer.
 *
 * The upload (device memory, 16-byte aligned, the caller's ONE copy): header blocks and entropy-coded segments at 16-byte offsets,
 * anywhere in it; two images may name the same header block.
 * The table block (n * SCG_JPEGDEC_IMAGE_WORDS + 3 (n + 1) uint32, little-endian; written by scg_jpegdec_batch_plan into host
 * memory, uploaded by the caller, normally at the front of the upload):
 *   n image records of SCG_JPEGDEC_IMAGE_WORDS words:
 *     [0, 16)    the frame
 *     [16]       bytes of the segment;  [17] 0
 *     [18, 24)   three uint64 (low word first): offset of the header block and of the segment in the upload, of the pixels in `out`
 *     [24, 44)   ten uint64: offsets in the workspace of the change counters, entry, exit, bnd, cnt, dcs, coefficients, and the
 *                planes Y, Cb, Cr (one component: all three name the Y plane)
 *     [44, 48)   0
 *   then three prefix tables of n + 1 words: the first workgroup of each image in the entropy grid, the idct grid and the colour
 *   grid; entry n is the grid's size.
 * The output: ONE buffer; image i holds its tight H W components bytes at its offset, every offset 16-byte aligned, the images in
 * input order, so images of one shape lie at a constant stride.
 * The workspace: 4 n status words first (four per image, as above), then the change counters of every image (one word per sync
 * launch, max_rounds of them; ONE clear covers both), then per image entry, exit, bnd, cnt, dcs and the planes, then every
 * coefficient buffer side by side (ONE clear).
 */
#ifndef SCG_JPEGDEC_H
#define SCG_JPEGDEC_H

#include "../scg_raster.h"

#define SCG_JPEGDEC_ABI_VERSION 2
#define SCG_JPEGDEC_SUBSEQ 128            /* bytes of a subsequence: one thread's share of the stream */
#define SCG_JPEGDEC_THREADS 256           /* threads of a workgroup of the entropy kernels */
#define SCG_JPEGDEC_MAX_DIM 65535         /* H and W */
#define SCG_JPEGDEC_MAX_SEGMENT 268435455 /* bytes of the entropy-coded segment: bit positions are 32-bit */
#define SCG_JPEGDEC_HEADER_BYTES 4096
#define SCG_JPEGDEC_FRAME_WORDS 16
#define SCG_JPEGDEC_IMAGE_WORDS 48            /* uint32 of an image record of the batch's table */
#define SCG_JPEGDEC_MAX_BATCH 65535           /* images of one scg_jpegdec_decode_batch */
#define SCG_JPEGDEC_BAD_CODE 1            /* a code word no table holds, or a size beyond 11 (DC) / 10 (AC) */
#define SCG_JPEGDEC_BAD_ZIGZAG 2          /* a run past coefficient 63 */
#define SCG_JPEGDEC_BAD_COUNT 4           /* the blocks found are not the frame's */
#define SCG_JPEGDEC_BAD_SYNC 8            /* the last sync launch still changed a state: run more rounds */
#define SCG_JPEGDEC_BAD_RESTART 16        /* a restart marker off its interval, out of order, or without DRI */

#ifdef __cplusplus
extern "C" {
#endif

SCG_API const char* scg_jpegdec_last_error(void);
SCG_API int32_t scg_jpegdec_abi_version(void);

/* Host only.  For a frame and the bytes of its entropy-coded segment: the workspace and the output in bytes, and the number of
 * sync launches after which the states are right, and seen to be, whatever the stream (the workgroups + 1; 1 with one workgroup). */
SCG_API int scg_jpegdec_sizes(const int32_t* frame, uint64_t segment_bytes, uint64_t* workspace_bytes, uint64_t* out_bytes,
                              int32_t* max_rounds);

/* header_dev: the header block; segment_dev[0, segment_bytes): the entropy-coded segment (behind SOS, up to the marker that ends
 * it), any alignment; out[0, out_bytes) with out_bytes >= H W components, 16-byte aligned; workspace[0, workspace_bytes),
 * 16-byte aligned.  rounds_done = 0 starts a decode and runs `rounds` >= 1 sync launches, then count, scan, write, idct, colour.
 * When the status has SCG_JPEGDEC_BAD_SYNC (its other bits then say nothing: the states they were found from are not settled), the
 * same call with rounds_done = the launches run so far continues with `rounds` more on the workspace as it stands and runs the
 * other kernels again.  rounds_done + rounds is at most scg_jpegdec_sizes' max_rounds: the one limit of both entries. */
SCG_API int scg_jpegdec_decode(const int32_t* frame, const void* header_dev, const uint8_t* segment_dev, uint64_t segment_bytes,
                               void* out, size_t out_bytes, void* workspace, size_t workspace_bytes, int32_t rounds_done,
                               int32_t rounds, void* stream);

/* Host only.  For n (1..SCG_JPEGDEC_MAX_BATCH) images — frames[n][SCG_JPEGDEC_FRAME_WORDS], segment_bytes[n], and per image the
 * 16-byte-aligned offset of its header block and of its segment in an upload of upload_bytes — the table block (above) into
 * table[0, table_words), each image's offset in the output into out_offsets[n], the workspace and output totals, and max_rounds:
 * the maximum over the images of scg_jpegdec_sizes' max_rounds. */
SCG_API int scg_jpegdec_batch_plan(int32_t n, const int32_t* frames, const uint64_t* segment_bytes, const uint64_t* header_offsets,
                                   const uint64_t* segment_offsets, uint64_t upload_bytes, uint32_t* table, uint64_t table_words,
                                   uint64_t* out_offsets, uint64_t* workspace_bytes, uint64_t* out_bytes, int32_t* max_rounds);

/* frames and table: the HOST copies, validated in full (every record and prefix entry must be what scg_jpegdec_batch_plan gives
 * for these frames and the offsets the records name, inside upload_bytes) before anything touches a device.  table_dev: the
 * uploaded table block, 16-byte aligned; upload_dev[0, upload_bytes), out[0, out_bytes) and workspace[0, workspace_bytes), each
 * 16-byte aligned and at least the plan's totals.  Runs `rounds` sync launches, 1 <= rounds <= max_rounds, then count, scan,
 * write, idct, colour, once for the whole batch.  There is no continuation: an image whose status carries SCG_JPEGDEC_BAD_SYNC is
 * the caller's to decode again (scg_jpegdec_decode). */
SCG_API int scg_jpegdec_decode_batch(int32_t n, const int32_t* frames, const uint32_t* table, const void* table_dev,
                                     const void* upload_dev, uint64_t upload_bytes, void* out, size_t out_bytes, void* workspace,
                                     size_t workspace_bytes, int32_t rounds, void* stream);

#ifdef __cplusplus
}
#endif
#endif
