/*
 * ug_mi355x.h -- C ABI of libug_mi355x.so, the MI355X (gfx950 / CDNA4) kernel library for
 * UltraGrid's per-frame pixel-format-conversion + block-compression hot path.
 *
 * This header is the drop-in boundary.  It replaces, for this path,
 *   - cuda_dxt/cuda_dxt.h:30-89      (cuda_{rgb,yuv}_to_dxt{1,6}, cuda_yuv422_to_yuv444)
 *   - src/cuda_wrapper.h:50-76       (device select / alloc / memcpy / last-error shim)
 *   - the per-line CPU decoder_t loop every compress module runs before upload
 *     (src/pixfmt_conv.h:87-88, src/video_compress/cuda_dxt.cpp:206-220,
 *      src/video_compress/dxt_glsl.cpp:277-289, src/video_compress/gpujpeg.cpp:592-608)
 *   - the packed->planar whole-buffer converters src/to_planar.h:53-74
 *   - the FDCT+quantise stage UltraGrid gets from libgpujpeg
 *     (src/video_compress/gpujpeg.cpp:617-631)
 *
 * Conventions (same as cuda_dxt.h): plain C, no C++ types, no ownership transfer (the
 * caller owns every buffer), every function returns 0 on success and a negative
 * UG_HIP_E* code on failure and never throws; distinct streams may be driven from
 * distinct threads concurrently.  Kernels are ASYNCHRONOUS on `stream` (unlike
 * cuda_dxt.cu:759, which synchronises after every launch) -- call ug_hip_stream_sync()
 * or order a D2H copy on the same stream.  `stream` == NULL is the device's null stream.
 *
 * Image geometry: `width`/`height` in pixels; a NEGATIVE height means the source image is
 * read bottom-up (vertical mirror), exactly as cuda_dxt.h:38-39.  `src_pitch` is the
 * source line stride in bytes; 0 selects the tightly packed UltraGrid line size
 * (vc_get_linesize, src/video_codec.c:507-521).
 *
 * Argument ranges: width and |height| from 1 to 65536 (UltraGrid's largest mode is 8K) and at most INT_MAX bytes per frame or plane
 * (pitch x lines).  Anything outside -- sizes that are not a picture, or whose byte counts would leave int / size_t range somewhere -- is
 * refused with UG_HIP_EINVAL before any device call (cuda_dxt.cu:745-746 returns -1 for a bad size); no entry point returns success, a
 * wrapped value or a runtime error for such input (tests/test_abi.py::test_absurd_geometry_is_refused, every entry point of this header).
 */
#ifndef UG_MI355X_H
#define UG_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UG_HIP_ABI_VERSION 5 /* 5: ug_hip_memcpy_2d_async, ug_hip_download_2d_ordered_ex, ug_hip_event_* / ug_hip_stream_wait_event, ug_hip_jpeg_encoder_create_ex, ug_hip_jpeg_colour_* (additions), and the DXT encoder / decoders take ANY frame size (they refused sizes
                              * that are not multiples of 4; ug_hip_dxt_size rounds up to whole blocks as dxt_get_size does); 4: ug_hip_{upload,download}_ordered_ex (additions only); 2: tie-rule option (UG_DXT_TIES_*), default = ties to even; *_ex / batched entry points; 3: NUMA placement, de-interlace (additions), and ONE
                              * change of behaviour: ug_hip_jpeg_encoder_encode_batch with frames > 1 reports a stream that does not fit its slice through
                              * out_len[f] > out_capacity and returns success for the call (it used to fail the whole call with UG_HIP_EINVAL) */

/* error codes (cuda_dxt.cu:745-746,759 uses -1 bad size/alignment, -3 runtime failure) */
#define UG_HIP_SUCCESS      0
#define UG_HIP_EINVAL     (-1) /* bad size / alignment / NULL pointer */
#define UG_HIP_EUNSUPP    (-2) /* no kernel for this format pair */
#define UG_HIP_ERUNTIME   (-3) /* HIP runtime error: see ug_hip_last_error_string() */

typedef void *ug_hip_stream_t; /* == hipStream_t; replaces cuda_wrapper_stream_t */

/* Pixel formats (own numbering; UltraGrid codec_t values are mapped by the module shim,
 * ultragrid_amd/module/ug_codec_map.h). */
typedef enum {
        UG_PF_NONE = 0,
        UG_PF_RGBA = 1,     /* 8-bit R,G,B,A bytes (shifts configurable on output) */
        UG_PF_UYVY = 2,     /* 8-bit 4:2:2  U Y0 V Y1 */
        UG_PF_YUYV = 3,     /* 8-bit 4:2:2  Y0 U Y1 V */
        UG_PF_RGB  = 4,     /* 8-bit R,G,B */
        UG_PF_BGR  = 5,     /* 8-bit B,G,R */
        UG_PF_V210 = 6,     /* 10-bit 4:2:2, 6 px / 16 B, lines padded to 128 B */
        UG_PF_RG48 = 7,     /* 16-bit little-endian R,G,B */
        UG_PF_YUV444 = 8,   /* packed 8-bit Y,U,V triplets (output of *_yuv422_to_yuv444) */
        UG_PF_UYVY_RAW = 9, /* UYVY fed to the encoder WITHOUT colour conversion (DXT1_YUV) */
        UG_PF_I420 = 10,    /* planar 4:2:0: Y, U, V planes back to back (JPEG encoder input only) */
        /* the other codecs of decoders[] (pixfmt_conv.c:3041-3103), ug_hip_pixfmt_convert only: */
        UG_PF_R10K = 11,    /* 10-bit RGB, 4 B / px big-endian, lines padded to 64 px (types.h R10k) */
        UG_PF_R12L = 12,    /* 12-bit RGB, 8 px / 36 B little-endian bit stream (R12L) */
        UG_PF_Y216 = 13,    /* 16-bit 4:2:2  Y0 Cb Y1 Cr */
        UG_PF_Y416 = 14,    /* 16-bit 4:4:4:4  U Y V A */
        UG_PF_VUYA = 15,    /* 8-bit 4:4:4:4  V U Y A */
        UG_PF_DVS10 = 16,   /* 10-bit 4:2:2 of DVS cards, 6 px / 16 B like v210 */
        /* an OUTPUT of ug_hip_pixfmt_convert[_batch] from UG_PF_RGB / UG_PF_RGBA only, no codec of its own (never an input, never a
         * ug_hip_pixfmt_best answer): UYVY bytes as dxt_compress/rgba_to_yuv422.glsl computes them -- the shader of `-c uyvy`
         * (src/video_compress/uyvy.cpp) -- lines of vc_get_linesize(width, UYVY) bytes */
        UG_PF_UYVY_GL = 17,
} ug_pixfmt_t;

typedef enum {
        UG_DXT1       = 1, /* 8 B / 4x4 block, output size w*h/2 (dxt_util.h:59-67) */
        UG_DXT1_YUV   = 2, /* DXT1 blocks holding Y,Cb,Cr (-c RTDXT:DXT1_YUV, types.h DXT1_YUV): encode takes UG_PF_UYVY only
                            * (== UG_PF_UYVY_RAW -> UG_DXT1), decode applies display_dxt1_yuv_fp.glsl */
        UG_DXT5_YCOCG = 6, /* "DXT6": 16 B / block, output size w*h */
} ug_dxt_t;

/* ------------------------------------------------------------------------------------
 * Runtime shim (replaces src/cuda_wrapper.h:50-76)
 * ---------------------------------------------------------------------------------- */
int         ug_hip_abi_version(void);
int         ug_hip_device_count(int *count);
/* 1 if ptr is device memory of this process (a device-resident video_frame, types.h:295-298 mem_location; the reference's
 * GPUJPEG module takes such frames without the upload, gpujpeg.cpp:617-622), 0 for host / unknown pointers. Never fails. */
int         ug_hip_pointer_is_device(const void *ptr);
/* index of the device that owns ptr, -1 for host / unknown pointers: a module state bound to device d reads a device-resident frame in
 * place only when this returns d (a frame that lives on another GPU is copied over first). Never fails. */
int         ug_hip_pointer_device(const void *ptr);
int         ug_hip_set_device(int index);                              /* cuda_wrapper_set_device */
int         ug_hip_malloc(void **buffer, size_t size);                 /* cuda_wrapper_malloc */
int         ug_hip_free(void *buffer);                                 /* cuda_wrapper_free */
int         ug_hip_malloc_host(void **buffer, size_t size);            /* cuda_wrapper_malloc_host (pinned) */
int         ug_hip_free_host(void *buffer);                            /* cuda_wrapper_free_host */
#define UG_HIP_MEMCPY_HOST_TO_DEVICE 0
#define UG_HIP_MEMCPY_DEVICE_TO_HOST 1
#define UG_HIP_MEMCPY_DEVICE_TO_DEVICE 2
int         ug_hip_memcpy(void *dst, const void *src, size_t count, int kind);       /* cuda_wrapper_memcpy */
int         ug_hip_memcpy_async(void *dst, const void *src, size_t count, int kind, ug_hip_stream_t stream);
/* `rows` lines of `width_bytes` bytes, `spitch` / `dpitch` bytes from one line to the next: ONE copy for a picture whose pitch differs from its
 * line size (the receivers' display pitch: src/video_decompress/dxt_glsl.c:163-186, gpujpeg.c:305-315 loop over the lines on the CPU there).
 * 0 < width_bytes <= both pitches, 0 < rows <= 65536, else UG_HIP_EINVAL before any device call. */
int         ug_hip_memcpy_2d_async(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width_bytes, size_t rows, int kind, ug_hip_stream_t stream);
int         ug_hip_memset_async(void *dst_dev, int value, size_t count, ug_hip_stream_t stream); /* device memory only */
/* Copy lanes: the copy goes onto the ONE upload (download) stream of `device` -- shared by every caller in the process, so that concurrent
 * frames do not split the link between two copies of the same direction -- and is ordered against `stream`: an upload starts after what
 * `then_stream` holds so far and `then_stream` continues after it; a download starts after what `after_stream` holds so far, and
 * ug_hip_stream_sync(after_stream) also waits for it.  The calling thread's current device must be `device`. */
int         ug_hip_upload_ordered(int device, void *dst_dev, const void *src, size_t count, int kind, ug_hip_stream_t then_stream);
int         ug_hip_download_ordered(int device, void *dst_host, const void *src_dev, size_t count, ug_hip_stream_t after_stream);
/* The same with one half of the ordering left to the caller -- what a frame cut into row bands needs (module option bands=<k>: upload of band k+1,
 * kernels of band k and download of band k-1 at the same time, inside ONE frame; the tile fan-out of video_compress.cpp:441-490 is the reference's
 * only intra-frame parallelism):
 *   UG_HIP_COPY_NO_WAIT  upload: the lane does NOT wait for what `then_stream` holds (the caller knows the destination is not in use any more, e.g. the
 *                        next band of a frame whose first band's upload did wait); `then_stream` still continues after the copy
 *   UG_HIP_COPY_NO_JOIN  download: `after_stream` does NOT wait for the copy (its later kernels run beside it); the lane is in order, so a later
 *                        download on the same device WITHOUT this flag makes ug_hip_stream_sync(after_stream) wait for this one too */
#define UG_HIP_COPY_NO_WAIT 1
#define UG_HIP_COPY_NO_JOIN 2
int         ug_hip_upload_ordered_ex(int device, void *dst_dev, const void *src, size_t count, int kind, ug_hip_stream_t then_stream, int flags);
int         ug_hip_download_ordered_ex(int device, void *dst_host, const void *src_dev, size_t count, ug_hip_stream_t after_stream, int flags);
/* the download lane with a 2-D copy (a row band of a picture with a display pitch): geometry as ug_hip_memcpy_2d_async, ordering and flags as above */
int         ug_hip_download_2d_ordered_ex(int device, void *dst_host, size_t dpitch, const void *src_dev, size_t spitch, size_t width_bytes, size_t rows,
                                          ug_hip_stream_t after_stream, int flags);
/* Events (hipEvent_t, timing disabled): record a point of one stream, make another stream wait for it.  What lets a second host thread
 * download the first bands of a picture while the first thread still uploads its last ones (copies from / to pageable host memory block the
 * calling thread: only two threads ever have an upload and a download in flight together). */
typedef void *ug_hip_event_t;
int         ug_hip_event_create(ug_hip_event_t *event);
int         ug_hip_event_destroy(ug_hip_event_t event);                /* NULL: nothing to do */
int         ug_hip_event_record(ug_hip_event_t event, ug_hip_stream_t stream);
int         ug_hip_stream_wait_event(ug_hip_stream_t stream, ug_hip_event_t event);
int         ug_hip_stream_create(ug_hip_stream_t *stream);
int         ug_hip_stream_destroy(ug_hip_stream_t stream);
int         ug_hip_stream_sync(ug_hip_stream_t stream);
const char *ug_hip_last_error_string(void);                            /* cuda_wrapper_last_error_string */
/* NUMA placement of the host threads that feed a GPU (the reference has one worker thread per device, gpujpeg.cpp:446-466, and leaves
 * its placement to the scheduler; on a two-socket, eight-GPU node that is the host-side limit SURVEY.md 8(e) expects).
 * ug_hip_device_numa_node: *node = NUMA node of the device's PCI function (sysfs numa_node), -1 if the platform does not say.
 * ug_hip_bind_thread_to_device: restricts the CALLING THREAD to the CPUs of that node (intersected with its current affinity, never
 * widened); *cpus_bound = CPUs it now runs on, 0 if it was left alone (unknown node, empty intersection).  Call it before the thread
 * allocates its pinned buffers, so that they are first touched on that node.  The *_of_pci / *_to_numa_node forms take the PCI
 * address / node directly and an alternative sysfs root (NULL = "/sys"): what the two above are made of, testable without a GPU. */
int         ug_hip_device_numa_node(int device, int *node);
int         ug_hip_bind_thread_to_device(int device, int *cpus_bound);
int         ug_hip_numa_node_of_pci(const char *bdf, const char *sysfs_root, int *node);
int         ug_hip_bind_thread_to_numa_node(int node, const char *sysfs_root, int *cpus_bound);
/* Average duration in milliseconds of `iters` back-to-back launches of the DXT encoder on
 * `stream`, measured with hipEvents on that stream (cuda_dxt/rgb2dxt1.c:87-108 is the
 * reference's equivalent harness).  Writes ms per launch to *ms_per_launch. */
int         ug_hip_time_dxt_encode(ug_pixfmt_t in, ug_dxt_t out, const void *src, void *dst, int width,
                                   int height, int src_pitch, int frames, size_t src_frame_stride,
                                   size_t dst_frame_stride, int iters, ug_hip_stream_t stream,
                                   float *ms_per_launch);

/* ------------------------------------------------------------------------------------
 * DXT encoders (replace cuda_dxt/cuda_dxt.h:30-89)
 * ---------------------------------------------------------------------------------- */
/* The reference's normative encoders are GLSL shaders (dxt_compress/compress_dxt5ycocg_fp.glsl, compress_dxt1_fp.glsl), and GLSL
 * leaves two things they use to the implementation: the direction of exact .5 ties of round() and the order in which dot(vec3)
 * is summed.  The choice is a run-time option:
 *   UG_DXT_TIES_EVEN  (default) round() ties to even, dot(vec3) summed from the last component: what the shaders compute where
 *                     they can actually be EXECUTED -- Mesa llvmpipe; every block of tests/golden/dxt_glsl_ref.npz (generated by
 *                     running the reference's shader files) is reproduced in this mode.  On the decode side: float -> unorm8
 *                     framebuffer writes of rgba_to_yuv422.glsl / display_dxt1_yuv_fp.glsl tie to even (Mesa again).
 *   UG_DXT_TIES_AWAY  roundf() half away from zero, dot() left to right: the reference's CUDA text (cuda_dxt.cu:106-108,
 *                     122-124), which cannot be executed here; decode side: floor(x * 255 + 0.5).
 * The two differ in ~0.3 % of uniform-random blocks (one endpoint LSB or one palette index). */
#define UG_DXT_TIES_EVEN    0
#define UG_DXT_TIES_AWAY    1
#define UG_DXT_TIES_DEFAULT UG_DXT_TIES_EVEN

/* Fused pixel-format unpack + colour conversion + 4x4 block encode, one pass, no
 * intermediate buffer.  `in` in {RGB, RGBA, UYVY, UYVY_RAW, V210, YUV444}.
 * Requirements: src 16-B aligned, dst 16-B aligned, pitch % 4 == 0 (V210: pitch % 16 == 0 and >= 32 * ceil(width / 12), which
 * vc_get_linesize's 128-byte padding always satisfies; the partial last 12-pixel unit of a line is read whole and encoded in part).
 * ANY width and |height| >= 1 is taken, as dxt_encoder_create does (dxt_compress/dxt_encoder.c:235, called with any tile size by
 * src/video_compress/dxt_glsl.cpp:150-160): the stream holds (width+3)/4 x (height+3)/4 blocks (dxt_get_size, dxt_util.h:59-67);
 * columns past the picture repeat its last column -- the shaders' GL_CLAMP_TO_EDGE fetches (dxt_encoder.c:362-364,
 * compress_dxt5ycocg_fp.glsl:45-55,341), bit for bit -- and lines past the picture repeat its last line (the one deliberate deviation:
 * the reference resamples such a picture vertically and leaves the last block row unrendered, dxt_encoder.c:380 vs :393,653-671;
 * INTEGRATION.md).  With a width that is not a multiple of 4, RGB / YUV444 lines may have any pitch (3 * width bytes), RGBA and
 * UYVY pitch % 4 == 0.  UYVY / V210 need an even width.  These use UG_DXT_TIES_DEFAULT. */
int ug_hip_dxt_encode(ug_pixfmt_t in, ug_dxt_t out, const void *src_dev, void *dst_dev,
                      int width, int height, int src_pitch, ug_hip_stream_t stream);
/* Same, `frames` images per launch (tiles of one frame or consecutive frames):
 * image i at src + i*src_frame_stride -> dst + i*dst_frame_stride. */
int ug_hip_dxt_encode_batch(ug_pixfmt_t in, ug_dxt_t out, const void *src_dev, void *dst_dev,
                            int width, int height, int src_pitch, int frames,
                            size_t src_frame_stride, size_t dst_frame_stride,
                            ug_hip_stream_t stream);
/* Same with the tie rule given explicitly (UG_DXT_TIES_*; anything else: UG_HIP_EINVAL). */
int ug_hip_dxt_encode_batch_ex(ug_pixfmt_t in, ug_dxt_t out, const void *src_dev, void *dst_dev,
                               int width, int height, int src_pitch, int frames,
                               size_t src_frame_stride, size_t dst_frame_stride, int ties,
                               ug_hip_stream_t stream);
/* bytes produced for one image: ((width+3)/4*4) * ((|height|+3)/4*4), half of it for DXT1 (dxt_get_size, dxt_util.h:59-67) */
size_t ug_hip_dxt_size(ug_dxt_t out, int width, int height);

/* Signature-compatible counterparts of cuda_dxt.h (src = tightly packed 3 B/px device
 * buffer; cuda_yuv_* take packed Y,U,V triplets).  These are asynchronous too.  They keep that interface's limits: size_x and
 * |size_y| must be multiples of 4 (cuda_dxt.cu:745 returns -1 otherwise; here UG_HIP_EINVAL). */
int ug_hip_rgb_to_dxt1(const void *src, void *out, int size_x, int size_y, ug_hip_stream_t stream); /* cuda_rgb_to_dxt1, cuda_dxt.h:41 */
int ug_hip_yuv_to_dxt1(const void *src, void *out, int size_x, int size_y, ug_hip_stream_t stream); /* cuda_yuv_to_dxt1, cuda_dxt.h:62 */
int ug_hip_rgb_to_dxt6(const void *src, void *out, int size_x, int size_y, ug_hip_stream_t stream); /* cuda_rgb_to_dxt6, cuda_dxt.h:83 */
int ug_hip_yuv_to_dxt6(const void *src, void *out, int size_x, int size_y, ug_hip_stream_t stream); /* cuda_yuv_to_dxt6, cuda_dxt.h:86 */
int ug_hip_yuv422_to_yuv444(const void *src, void *out, int pix_count, ug_hip_stream_t stream);     /* cuda_yuv422_to_yuv444, cuda_dxt.h:88 */

/* ------------------------------------------------------------------------------------
 * DXT decoders (receiver side; replace dxt_decoder_decompress() behind
 * src/video_decompress/dxt_glsl.c:142-189 and the CPU tool cuda_dxt/dxt62tga.c:24-106)
 * ---------------------------------------------------------------------------------- */
/* `in` in {UG_DXT1, UG_DXT5_YCOCG}; `out` in {UG_PF_RGB, UG_PF_BGR, UG_PF_RGBA, UG_PF_UYVY}.  RGBA output honours
 * rshift/gshift/bshift exactly like the decompress modules' reconfigure() arguments (video_decompress.h:85-100);
 * UYVY follows dxt_compress/rgba_to_yuv422.glsl.  dst_pitch 0 = packed.  Any width, height >= 1 (UYVY: even width): the stream
 * holds (width+3)/4 x (height+3)/4 blocks, width x height pixels are written (dxt_compress/dxt_decoder.c:146-149,368-389).
 * Pitch and alignment: dst_dev is 16-byte aligned, src_dev 16-byte (DXT5) or 8-byte (DXT1, DXT1_YUV) aligned.  dst_pitch is at least the
 * line (4, 3, 3, 2 bytes per pixel) and, with width and height both multiples of 4, a multiple of 16 (RGBA), 8 (UYVY) or 4 (RGB, BGR) --
 * a row of a block leaves as one 128-, 64- or 32-bit store; with any other size a multiple of 4 (RGBA, UYVY) or any value (RGB, BGR).
 * Only the width x height pixels are written: line padding and whatever follows the last line stay as they were.  Anything else is
 * UG_HIP_EINVAL, and nothing is written. */
int ug_hip_dxt_decode(ug_dxt_t in, ug_pixfmt_t out, const void *src_dev, void *dst_dev, int width, int height,
                      int dst_pitch, int rshift, int gshift, int bshift, ug_hip_stream_t stream);
/* Same with the tie rule given explicitly (UG_DXT_TIES_*): it decides the float -> unorm8 writes of the UYVY output pass and of the
 * DXT1_YUV display matrix; the other outputs do not depend on it. */
int ug_hip_dxt_decode_ex(ug_dxt_t in, ug_pixfmt_t out, const void *src_dev, void *dst_dev, int width, int height,
                         int dst_pitch, int rshift, int gshift, int bshift, int ties, ug_hip_stream_t stream);
/* Device self-test: the decoders divide by the constants 255, 31, 63, 7, 5, 3 with a multiply + two fma (correctly rounded for
 * the numerators a DXT block can produce); this compares every such quotient with the IEEE division. *mismatches must be 0. */
int ug_hip_selftest_dxt_decode(unsigned *mismatches, ug_hip_stream_t stream);
/* Diagnostics (tests, profiling): which DXT5-YCoCg decode path the following ug_hip_dxt_decode calls of this process take --
 * 0 = the product (32-bit fixed point with a guard band; blocks with a value inside the band are decoded again with dxt62tga.c's fp64
 * statements: bit-identical by construction), 1 = the fp64 statements only, 2 = fixed point only (no fallback: shows what the guard is
 * for) -- and, if not NULL, a device counter that every guarded block increments.  Reset with (0, NULL). */
int ug_hip_dxt_decode_debug(int mode, unsigned *flagged_blocks_dev);
/* Same for the encoder: x / 14.0f as multiply + two fma, compared with the IEEE division for x = 0 and every fp32 x in [2^-100, 1] (smaller
 * values take the division itself). */
int ug_hip_selftest_dxt_encode(unsigned *mismatches, ug_hip_stream_t stream);
/* Diagnostics (tests, profiling).  The encoders choose each pixel's ONE decisive comparison of compress_dxt5ycocg_fp.glsl:237-244 /
 * :262-312 from the pixel's position on the palette segment / among the alpha thresholds and evaluate that comparison exactly as the
 * reference does; a wave that holds a block outside the precondition (coincident colour end points over non-flat chroma; luma range < 2^-10) evaluates the
 * reference's full form for all of its blocks.  Returns the number of such waves since the last reset on the current device:
 * [0] colour stage, [1] alpha stage.  Synchronises the device. */
int ug_hip_dxt_encode_stats(unsigned long long full_form_waves[2], int reset);
/* The same with a third count.  From a 4:2:2 source (UYVY, v210) the DXT5-YCoCg encoder takes the sign of SelectYCoCgDiagonal's
 * covariance (glsl:169-183) from one product per chroma pair wherever an error bound decides it; a wave that holds a block the bound
 * does not decide forms the reference's 16-term sum for all of its blocks.  In the same way its colour stage takes the colour index
 * of a chroma pair (glsl:231-244) from the projection of the pair's even pixel on the palette segment wherever an error bound decides it
 * for both pixels; a wave that holds a pair the bound does not decide evaluates the reference's two squared distances for the pixels of
 * the pair slots that hold such a pair.  counts[0 .. n - 1], n = 0 .. 4, receive { colour full form, alpha full form, waves that formed the reference's
 * covariance sum, waves that evaluated per-pixel distances after the projection }.  A reset through either function clears all four. */
int ug_hip_dxt_encode_stats_ex(unsigned long long *counts, int n, int reset);
/* A fifth count, through an entry point of its own (the one above keeps refusing n > 4).  From a 4:2:2 source the DXT5-YCoCg encoder
 * takes the 3-bit alpha count of a pixel (glsl:262-312) from the pixel's location among the thresholds, RN(7 - (a - min) * 7 / range),
 * wherever an error bound keeps every pixel of the block away from a threshold; a wave that holds a block the bound does not decide
 * forms the reference's thresholds and evaluates the reference's comparison for every pixel of all of its blocks.  *exact_waves (may be
 * NULL) receives the number of such waves since the last reset on the current device.  Content with flat chroma and few luma levels
 * puts a pixel on the middle threshold in most blocks: there every wave counts.  A reset through any of the stats functions clears all
 * counts.  Synchronises the device. */
int ug_hip_dxt_encode_stats_alpha(unsigned long long *exact_waves, int reset);
/* A sixth count, of the work behind counts[3] above.  A block holds eight chroma pairs, pair slots 0 .. 7.  A wave that holds an
 * uncertified pair keeps the projection's index for every certified pair and evaluates the reference's distances for the two pixels of
 * each pair slot in which one of its blocks holds an uncertified pair.  *slot_evaluations (may be NULL) receives the number of such
 * (wave, slot) evaluations since the last reset on the current device: between 1 and 8 for every wave of counts[3].  A reset through
 * any of the stats functions clears all counts.  Synchronises the device. */
int ug_hip_dxt_encode_stats_pair_slots(unsigned long long *slot_evaluations, int reset);
/* Diagnostics (tests, profiling): what the last call of an LDGM session (below) issued -- kernel launches, host <-> device copies (the
 * schedule upload included) and levels of its decode schedule.  Any pointer may be NULL.  Does not touch the device. */
typedef struct ug_hip_ldgm ug_hip_ldgm;
int ug_hip_ldgm_stats(const ug_hip_ldgm *s, int *launches, int *copies, int *levels);

/* ------------------------------------------------------------------------------------
 * LDGM forward error correction (replaces ldgm/src/ldgm-session-gpu.cpp + gpu.cu; the coder of src/rtp/ldgm.cpp)
 * ---------------------------------------------------------------------------------- */
/* A session holds one parity-check matrix on one device: `pcm` is m rows of w_f ints padded with -1 (LDGM_session::set_pcMatrix,
 * ldgm-session.cpp:40-121); row r lists its data packets (< k), then parity packets k + r and k + r - 1.  k 1..8191, m 1..65535, w_f 2..128,
 * every entry in [-1, k + m): anything else is refused with UG_HIP_EINVAL before the device is touched (so is a NULL pointer).
 * A buffer is k data packets of ps bytes followed by m parity packets; ps must be a positive multiple of 4 up to 65535 (LDGM_session's
 * packet_size is an unsigned short), else UG_HIP_EINVAL before any device call.  Calls switch to the session's device and back.
 * One session serves one call at a time; distinct sessions may run on distinct streams (and threads) at once.  Buffers the session keeps
 * for itself grow with the largest ps seen (hipMalloc: that call synchronises the device). */
int  ug_hip_ldgm_create(int device, int k, int m, const int *pcm, int w_f, ug_hip_ldgm **out);
void ug_hip_ldgm_destroy(ug_hip_ldgm *s); /* waits for the session's last schedule upload; NULL: nothing to do */
/* Encode: parity = the staircase of LDGM_session_cpu::encode (ldgm-session-cpu.cpp:152), byte for byte, written over the parity region of
 * `buf_dev` ((k + m) x ps bytes of device memory).  Two kernel launches on `stream`, asynchronous. */
int  ug_hip_ldgm_encode(ug_hip_ldgm *s, void *buf_dev, int ps, ug_hip_stream_t stream);
/* Decode in place on the device.  received[i] != 0: packet i (k + m of them) arrived whole.  The packets that can be recovered are found on
 * the host by peeling to the fixpoint (LDGM_session_cpu::decode_frame stops after 4 sweeps: this recovers every packet those do, and
 * possibly more); only the recoveries that missing data packets need are run, one kernel launch per level of the schedule, asynchronous on
 * `stream`.  recovered (k + m bytes, may be NULL) = 1 for each packet written: the recovered data packets and the parity packets rebuilt on
 * the way.  *all_data_known (may be NULL) = every data packet arrived or was recovered.  Packets that arrived are never written; missing
 * packets that are not recovered keep whatever the buffer held.  No data packet missing, or none recoverable: no device work at all.
 * The schedule goes up through a pinned staging buffer of the session: a call waits for the previous call's upload of it. */
int  ug_hip_ldgm_decode(ug_hip_ldgm *s, void *buf_dev, int ps, const uint8_t *received, uint8_t *recovered, int *all_data_known,
                        ug_hip_stream_t stream);
/* Host-buffer forms (the ldgm_gpu plugin): the same on a host buffer of (k + m) x ps bytes (pinned memory is copied fastest), through a
 * device buffer of the session.  Both synchronise `stream` before they return.
 *   encode_host: uploads the k x ps data bytes, downloads the m x ps parity bytes into buf_host.
 *   decode_host: with a data packet missing and recoverable, uploads the buffer, runs the schedule and downloads the recovered data
 *                packets only (gathered into one copy) into their places in buf_host; otherwise does nothing on the device. */
int  ug_hip_ldgm_encode_host(ug_hip_ldgm *s, void *buf_host, int ps, ug_hip_stream_t stream);
int  ug_hip_ldgm_decode_host(ug_hip_ldgm *s, void *buf_host, int ps, const uint8_t *received, uint8_t *recovered, int *all_data_known,
                             ug_hip_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Pixel-format conversion, whole frame on the device (replaces the decoder_t line loop,
 * pixfmt_conv.h:87-88 / pixfmt_conv.c:3041-3125)
 * ---------------------------------------------------------------------------------- */
/* 1 if a kernel exists for in -> out: every pair of decoders[] (== get_decoder_from_to(in, out) != NULL, pixfmt_conv.c:3110-3125) and in == out */
int ug_hip_pixfmt_supported(ug_pixfmt_t in, ug_pixfmt_t out);
/* get_best_decoder_from (pixfmt_conv.c:3126-3172): `candidates` ends with UG_PF_NONE; *out = the candidate the reference's ranking
 * (compare_pixdesc, video_codec.c:1148-1192: keep depth, then subsampling, then colour space; ties to the lower codec_t) puts first among
 * those reachable from `in`.  UG_HIP_EUNSUPP if none is reachable. */
int ug_hip_pixfmt_best(ug_pixfmt_t in, const ug_pixfmt_t *candidates, ug_pixfmt_t *out);
/* rshift/gshift/bshift have decoder_t meaning (honoured for RGBA / RGB outputs, defaults
 * 0/8/16, pixfmt_conv.h:62-65).  Pitches 0 = vc_get_linesize().
 * out = UG_PF_UYVY_GL (in = UG_PF_RGB or UG_PF_RGBA; any other input, or UG_PF_UYVY_GL as input: UG_HIP_EUNSUPP): output pixel pair i of
 * a line = rgba_to_yuv422.glsl's fp32 arithmetic on pixels 2i and 2i + 1 (for odd widths the last pair repeats the last pixel, GL's
 * CLAMP_TO_EDGE), float -> unorm8 with ties to even, alpha ignored, lines read at the given pitch (packed: 3 / 4 bytes per pixel).
 * Pitch and alignment: a pitch is at least vc_get_size(width, format); bytes [0, vc_get_size(width, out)) of a destination line are the
 * converter's, the rest of the pitch and everything around the picture is never written.  Alignment decides the speed, not the result:
 *   - the pairs among v210, UYVY, YUYV, RGB, BGR, RGBA and RG48 -> UYVY (and in == out) take any base address and any pitch;
 *   - in the other pairs of decoders[] the formats addressed as 16- or 32-bit words need base AND pitch aligned to them (as the reference
 *     asserts): 4 bytes for a v210 / DVS10 source and for an RGBA, UYVY, VUYA, v210 or R10k destination (R10k from R12L / Y416: bytes),
 *     2 bytes for RG48, Y216, Y416 on either side; RGB, R12L, and RGBA / UYVY / YUYV / VUYA / R10k / R12L sources are bytes.
 *     A call below that is refused with UG_HIP_EINVAL and writes nothing;
 *   - the 128-bit kernels run when both bases and both pitches are 16-byte aligned (a ragged end of the line, or the whole line
 *     otherwise, takes the byte- and word-wise kernels: same bytes). */
int ug_hip_pixfmt_convert(ug_pixfmt_t in, ug_pixfmt_t out, const void *src_dev, void *dst_dev,
                          int width, int height, int src_pitch, int dst_pitch,
                          int rshift, int gshift, int bshift, ug_hip_stream_t stream);
/* `frames` images per call, image i at src + i * src_frame_stride -> dst + i * dst_frame_stride.  When the frames follow each other
 * exactly one picture apart on both sides (stride == pitch * height: tiles, frame rings) the batch is ONE launch -- a 4K frame is a
 * 7-13 us launch, which cannot fill 256 CUs on its own; other layouts are converted frame by frame. */
int ug_hip_pixfmt_convert_batch(ug_pixfmt_t in, ug_pixfmt_t out, const void *src_dev, void *dst_dev, int width, int height,
                                int src_pitch, int dst_pitch, int rshift, int gshift, int bshift, int frames,
                                size_t src_frame_stride, size_t dst_frame_stride, ug_hip_stream_t stream);
/* The line converters pixfmt_conv.h:93-101 exports outside decoders[] (their callers reach them by name, e.g. video_capture/screen_x11.c:463,
 * decklink.cpp:1750), whole frame, line by line with the given dst_len (bytes to write per line) and pitches:
 *   "vc_copylineUYVYtoGrayscale" (:927-938), "vc_copylineABGRtoRGB" (:809-843), "vc_copylineBGRAtoRGB" (:845-857),
 *   "vc_copylineToRGBA_inplace" (:907-921; rshift/gshift/bshift are the SOURCE shifts, alpha byte 0; dst may equal src). */
int ug_hip_pixfmt_line_func(const char *func, const void *src_dev, void *dst_dev, int width, int height, int src_pitch, int dst_pitch, int dst_len,
                            int rshift, int gshift, int bshift, ug_hip_stream_t stream);
/* vc_get_linesize (video_codec.c:507-521) for the formats above; UG_HIP_EINVAL for an unknown format or a width outside 1..65536
 * (the reference's int arithmetic wraps there; this never returns a wrapped value) */
int ug_hip_linesize(ug_pixfmt_t fmt, int width);
/* vc_deinterlace (src/video_codec.c:597-664) IN PLACE on a device frame of `lines` lines of `linesize` bytes (pitch == linesize, as there):
 * the linear-blend de-interlace RTDXT applies to INTERLACED_MERGED input before encoding (dxt_glsl.cpp:195-201,291-293), computed as the
 * reference's x86-64 build computes it (its SSE2 bodies: a recursive pavgb blend down the lines; lines < 5: nothing) -- any line size from 16
 * bytes, including those that are no multiple of 16, whose last column reaches into the next line there.  linesize < 16 (where the reference's
 * 16-byte columns overlap themselves and, below 6 bytes, are stored past the frame): UG_HIP_EINVAL.  _batch: `frames` frames frame_stride apart. */
int ug_hip_deinterlace_blend(void *frame_dev, size_t linesize, int lines, ug_hip_stream_t stream);
int ug_hip_deinterlace_blend_batch(void *frame_dev, size_t linesize, int lines, int frames, size_t frame_stride, ug_hip_stream_t stream);

/* The `scale` video postprocessor (src/vo_postprocess/scale.c, `-p scale:<w>:<h>`): bilinear resampling of UG_PF_RGBA or UG_PF_UYVY pictures,
 * as the module's GL_LINEAR / GL_CLAMP_TO_EDGE texture draw computes it on Mesa llvmpipe (tests/golden/scale_gl_ref.npz) -- except next to position
 * ties, where llvmpipe's fp32 texture coordinates and the exact positions below can differ by one step: at most 1 LSB per byte.  A picture is a texture
 * of 4-byte texels -- one RGBA pixel, or one U Y0 V Y1 pair -- and with interlaced_merged two lines side by side form one texel row (twice as
 * wide, half as high: the vertical filter stays in one field), in and out (scale.c:190-216).  Per axis, n_in -> n_out texels, output texel x:
 *   p = round_half_up((2x + 1) * n_in * 128 / n_out) - 128;  i0 = p >> 8, i1 = i0 + 1 (both clamped to 0 .. n_in - 1);  w = p & 255
 *   lerp(a, b, w) = (a * (256 - w) + b * w + 128) >> 8 per byte; rows after columns.  A downscale by more than 2 still reads 2 x 2 texels.
 * Deviations from the reference's slips: a UYVY line is (width + 1) / 2 texels (vc_get_linesize), in and out (the reference's
 * textures are width / 2 texels wide and its rows shear); interlaced_merged with an odd dst_height is refused (the reference leaves the last line
 * unwritten); an odd src_height drops the last line, as there.
 * Pitches 0 = vc_get_linesize; otherwise at least that and a multiple of 4; pointers 4-byte aligned; lines past the written line size keep their
 * bytes.  Sizes 1..65536, at most INT_MAX bytes per frame, frames 1..65535 (grid.z), frame i at src + i * src_frame_stride -> dst + i *
 * dst_frame_stride (strides multiples of 4 covering a frame).  Anything else: UG_HIP_EINVAL (format: UG_HIP_EUNSUPP) before any device call. */
struct ug_scale_desc {
        const void *src;            /* device */
        void       *dst;            /* device */
        ug_pixfmt_t format;         /* UG_PF_RGBA or UG_PF_UYVY */
        int         interlaced_merged;
        int         src_width, src_height, dst_width, dst_height; /* pixels */
        size_t      src_pitch, dst_pitch;                         /* bytes per line */
        int         frames;
        size_t      src_frame_stride, dst_frame_stride;
};
int ug_hip_scale(const struct ug_scale_desc *d, ug_hip_stream_t stream);

/* The de-interlacing postprocessors / capture filters (`-p deinterlace`, `deinterlace_blend`, `double_framerate[:d]`, `deinterlace_bob`,
 * `deinterlace_linear`) on device frames of `lines` lines of `linesize` bytes, byte for byte what the reference's C computes:
 *   UG_DEINT_BLEND   vc_deinterlace_ex (src/video_codec.c:722-854): dst[0] line y = (a + b + 1) >> 1 of src lines y and y + 1 per element, the last
 *                    line = the destination's line above it; a single line is copied.  dst[0] may equal src (same pitch), as there.
 *   UG_DEINT_WEAVE   perform_df (src/vo_postprocess/temporal-deint.c:240-277): dst[0] = even lines of src + odd lines of prev (the frame before),
 *                    dst[1] = src; blend_after_weave (`:d`): vc_deinterlace_ex over each, in the same launch.
 *   UG_DEINT_BOB     perform_bob (:279-300): dst[0] = every even line twice; dst[1] = line 1, then every odd line twice; where the height
 *                    leaves a single last line it repeats the line above it.
 *   UG_DEINT_LINEAR  perform_linear (:442-466): as BOB with the lines between two field lines interpolated by avg_lines (:307-440); the last
 *                    one or two lines are copies of ONE source line, the first of them (the reference's source pointer stands still, :462-465).
 * Elements: bytes (RGBA, UYVY, YUYV, RGB, BGR, VUYA), uint16_t (RG48, Y216, Y416), v210's three fields per word (10, 10 and -- as `v >> 20` --
 * 12 bits), R10k's big-endian fields at bits 22 / 12 / 2 (the low two bits of every averaged word are zero, :797-803), R12L's stream of 12-bit
 * samples (:807-846).  avg_lines of the 8- and 16-bit formats is NOT that average but (c1 >> 1) + (c2 >> 1) + (c1 & 1), c1 the upper line
 * (temporal-deint.c:318-319,334-335), and its R10k words are read with ntohl but stored
 * in host order (:388-393: the averaged lines of LINEAR come out byte-swapped): both reproduced.  Any other format: UG_HIP_EUNSUPP (the reference returns false; its modules copy / bob).
 * An averaged line writes what the reference's loops reach and leaves the rest of the destination line as it was (WEAVE + blend: the woven bytes):
 *   BLEND: v210 / R10k linesize / 16 * 16 bytes; 16-bit formats the same from 16 bytes on (the x86-64 build's tail loop, :759,769, compares a
 *   byte offset with an element count and never runs behind its vector loop); R12L linesize / 36 groups of 8 words (a 36-byte group has 9: the last ninth of a line is
 *   never written, :814-816), less the last word where it ends inside a sample.  LINEAR: v210 the same; R12L linesize / 16 groups of 4 words.
 * Deviations, where the reference leaves its buffers: LINEAR R10k averages the one line (avg_lines walks four lines' worth,
 * :385-387); 8- / 16-bit LINEAR writes linesize bytes (avg_lines_per_elem rounds up to 16, :314,330); WEAVE with an odd number of lines
 * (:247-258) and BOB / LINEAR / WEAVE with one line are refused; lines == 0 (`lines - 1` underflows, :733) is refused; WEAVE + blend honours
 * dst_pitch (the reference passes the line size as pitch, :270-273).
 * Pitches 0 = linesize, otherwise at least that; linesize, pitches, strides and pointers multiples of the element size (1, 2, or 4 bytes for
 * v210 / R10k / R12L); lines 1..65536, at most INT_MAX bytes per frame, frames 1..65535 (grid.z), frame i at src (prev) + i * src_frame_stride
 * -> dst[k] + i * dst_frame_stride.  Sources and destinations must not overlap (but BLEND's dst[0] == src).  Anything else: UG_HIP_EINVAL
 * before any device call.  16-byte aligned pointers, pitches and strides take the dwordx4 path. */
#define UG_DEINT_BLEND  0
#define UG_DEINT_WEAVE  1
#define UG_DEINT_BOB    2
#define UG_DEINT_LINEAR 3
struct ug_deinterlace_desc {
        const void *src;            /* device: the frame */
        const void *prev;           /* device: the frame before it (WEAVE only; same pitch and stride as src) */
        void       *dst[2];         /* device: the output of postprocess(in) and of postprocess(NULL); BLEND writes dst[0] only */
        ug_pixfmt_t format;
        int         mode;           /* UG_DEINT_* */
        int         blend_after_weave;
        int         lines;
        size_t      linesize;       /* bytes */
        size_t      src_pitch, dst_pitch;
        int         frames;
        size_t      src_frame_stride, dst_frame_stride;
};
int ug_hip_deinterlace(const struct ug_deinterlace_desc *d, ug_hip_stream_t stream);
int ug_hip_deinterlace_supported(ug_pixfmt_t format, int mode); /* 1 / 0 */

/* The per-pixel colour filters and the two mirror filters (`-F` capture filters, and `-p` postprocessors through capture_filter_wrapper.h) on
 * device frames of `lines` lines of `width` pixels, byte for byte what the reference's C computes:
 *   UG_PXF_MATRIX   src/capture_filter/matrix.c:127-309: out = M * pixel, a 3x3 double matrix on unpacked components.  UG_PF_UYVY comes out as
 *                   UG_PF_RGB, 4 bytes -> 6, both pixels of a pair with the pair's U and V and the offsets -16 / -128 (:158-181); UG_PF_RGB and
 *                   UG_PF_RG48 keep their format.  clamp != 0: `int val = ...; CLAMP(val, 0, 255)` -- 0..255 for RG48's 16-bit elements too (:217);
 *                   clamp == 0 (`no-bound-check`, :95): the conversion below.
 *   UG_PXF_MATRIX2  src/capture_filter/matrix2.c:167-243: the matrix on offset Y / Cb / Cr.  UG_PF_UYVY: chroma from y = (y1 + y2) / 2, luma
 *                   from y1 and y2 (:174-196); UG_PF_Y416: offsets 1 << 15, 1 << 12, 1 << 15, alpha 0xFFFF (:219-237); UG_PF_V210: in one pass what
 *                   the reference does in three, vc_copylineV210toY416 (pixfmt_conv.c:2834-2882), that loop, vc_copylineY416toV210 (:3004-3031).
 *   UG_PXF_LUT      src/capture_filter/gamma.cpp:119-145: out[i] = lut[in[i]] per component; UG_PF_RGB (8 bits) or UG_PF_RG48 (16) in,
 *                   out_format UG_PF_RGB or UG_PF_RG48 out; lut_dev = a device table of 256 or 65536 uint8_t or uint16_t (ug_hip_gamma_lut fills
 *                   the host copy).  Every element is transformed (the reference's threads leave the last len % hardware_concurrency(), :133-138).
 *   UG_PXF_GRAY     src/capture_filter/grayscale.c:95-102: UG_PF_UYVY with U = V = 127.
 *   UG_PXF_MIRROR   src/capture_filter/mirror.c:76-93: a UG_PF_UYVY line reversed pair by pair, the two lumas of a pair swapped.
 *   UG_PXF_FLIP     src/capture_filter/flip.c:96-99: line y -> line lines - 1 - y; every packed format (not UG_PF_I420, UG_PF_UYVY_GL).
 * Arithmetic: integer -> double exact, IEEE fp64 products and sums in the reference's left-to-right order, never fused.  double -> integer: the
 * reference converts straight to unsigned char / uint16_t, undefined outside that type's range; here it is truncation toward zero to int32 and
 * then the low 8 or 16 bits, which is what its x86-64 build does.  So that the int32 step is defined, a matrix with a non-finite coefficient or a
 * row with sum |m| * (65535 + 32768) >= 2^31 is refused (UG_HIP_EINVAL).
 * A line is vc_get_linesize(format, width) bytes, all of it transformed (UYVY: whole pairs; v210: whole groups of the padded line -- the
 * reference hands the decoder the whole frame as one line, matrix2.c:216, which is the same only for widths that are multiples of 48).  MATRIX
 * on UYVY needs an even width.  out_format: UG_PF_NONE = the op's output format (MATRIX on UYVY: RGB; LUT: the input's), or that format named.
 * Pitches 0 = the line size, otherwise at least that; pitches, strides and pointers multiples of the element (2 bytes: RG48, Y416; 4: v210;
 * FLIP: 1); lines 1..65536, at most INT_MAX bytes per frame, frames 1..65535 (grid.z), frame i at src + i * src_frame_stride -> dst + i *
 * dst_frame_stride.  Source and destination must not overlap, whatever the op.  An op / format pair without a kernel: UG_HIP_EUNSUPP; anything
 * else: UG_HIP_EINVAL; both before any device call.  Units whose addresses are multiples of 16 take the dwordx4 path. */
#define UG_PXF_MATRIX  0
#define UG_PXF_MATRIX2 1
#define UG_PXF_LUT     2
#define UG_PXF_GRAY    3
#define UG_PXF_MIRROR  4
#define UG_PXF_FLIP    5
struct ug_pixel_filter_desc {
        const void *src;            /* device */
        void       *dst;            /* device */
        int         op;             /* UG_PXF_* */
        ug_pixfmt_t format;
        ug_pixfmt_t out_format;     /* UG_PF_NONE: the op's own */
        int         width, lines;   /* pixels, lines */
        size_t      src_pitch, dst_pitch;
        int         frames;
        size_t      src_frame_stride, dst_frame_stride;
        double      matrix[9];      /* MATRIX, MATRIX2: row-major [a b c; d e f; g h i] */
        int         clamp;          /* MATRIX: the bounds-checked form */
        const void *lut_dev;        /* LUT: device table */
};
int ug_hip_pixel_filter(const struct ug_pixel_filter_desc *d, ug_hip_stream_t stream);
int ug_hip_pixel_filter_supported(int op, ug_pixfmt_t format); /* 1 / 0 */
/* The tables of `gamma` (gamma.cpp:74-93): table_host[i] = pow(i / max_in, gamma) * max_out converted to uint8_t (out_bits 8) or uint16_t (16),
 * for i = 0 .. max_in, with the host's pow; in_bits and out_bits 8 or 16.  The caller uploads the table.  gamma <= 0 or not finite:
 * UG_HIP_EINVAL (the reference warns, :170-172, and goes on to convert inf). */
int ug_hip_gamma_lut(double gamma, int in_bits, int out_bits, void *table_host);
/* matrix2's named matrices (matrix2.c:69-73,113): "y601_to_y709".  Unknown name: UG_HIP_EINVAL. */
int ug_hip_matrix2_preset(const char *name, double m[9]);

/* Frame composition: the geometric and compositing postprocessors / capture filters on device frames of `lines` lines of `width` pixels, byte for
 * byte what the reference's C computes where that stays inside its buffers (the rest: "Deviations" below):
 *   UG_CMP_CROP           src/vo_postprocess/crop.c:159-182: dst line y = out_line_bytes bytes of src line yoff + y from byte xoff_bytes; out_lines
 *                         lines.  Works in bytes: every packed format.  ug_hip_crop_geometry gives the four numbers as the reference derives them.
 *   UG_CMP_BORDER         src/vo_postprocess/border.c:158-208: src copied, the top and bottom border_h lines and border_w pixels at either side filled
 *                         with `fill` (UG_PF_RGB: its first 3 bytes; UG_PF_RGBA: all 4; UG_PF_UYVY: the word U Y V Y, rows filled over the whole line
 *                         size, sides ceil(border_w / 2) pairs from each end).  ug_hip_border_pattern gives `fill` for a colour.
 *   UG_CMP_LOGO           src/capture_filter/logo.c:182-230: the R,G,B,A overlay `logo` (device, logo_w x logo_h x 4 bytes) blended IN PLACE into dst
 *                         (src NULL or == dst) at pixel (rect_x, rect_y): per pixel the reference's decoder to 8-bit RGB, c = (c * (255 - a) + l * a) /
 *                         255, its coder back.  UG_PF_UYVY (Q14 both ways, the pair's chroma from both blended pixels; an odd logo_w re-encodes the
 *                         whole last pair, its second pixel unblended), UG_PF_RGB, UG_PF_RGBA (alpha comes back 0xFF), UG_PF_RG48 (the high bytes; the
 *                         low bytes come back 0).  The frame under the logo changes even where alpha is 0.  rect_x or rect_y < 0: success, nothing done
 *                         (logo.c:195-196).  ug_hip_logo_geometry gives the rectangle, the reference's rounding slip included.
 *   UG_CMP_INTERLACE      src/vo_postprocess/interlace.c:172-181: dst line i = line i of src (the first frame of the pair) for even i, of src2 for odd i.
 *   UG_CMP_INTERLACED_3D  src/vo_postprocess/3d-interlaced.c:152-169: dst line x = per BYTE (a + b + 1) >> 1 of lines (x / 2) * 2 and (x / 2) * 2 + 1 of
 *                         eye x % 2 (src = tile 0, src2 = tile 1), whatever the format, as pavgb does (wrong for v210's 10-bit fields, reproduced).
 *   UG_CMP_SPLIT          src/utils/vf_split.cpp:79-108: tile (tx, ty) of grid_x x grid_y at dst + (ty * grid_x + tx) * tile_stride, its lines tile_pitch
 *                         apart (0: vc_get_linesize(tile width)), each tile_width * get_bpp bytes from byte tx * that of the source line; tile_stride 0 =
 *                         tile_pitch * tile lines; dst_pitch is not used.  The grid must divide width and lines (UG_HIP_EINVAL); v210 / DVS10 / R12L tiles
 *                         must be whole pixel blocks (UG_HIP_EUNSUPP).
 * Deviations and refusals, where the reference leaves its buffers: LOGO blends every logo pixel over its own decoded frame pixel (the reference's RGB
 * segment is (logo_w + 1) / bb * bb pixels wide, logo.c:198-222: narrower than the logo for logo_w % 4 in {1, 2} on UYVY / RGBA, % 3 == 1 on RGB, % 6 not
 * in {0, 5} on RG48, where its blend runs into the next line and past the allocation); a LOGO rectangle that leaves the frame is refused (the
 * reference's rounding toward zero draws a logo up to bb - 1 pixels wider than the frame across the line ends); INTERLACED_3D writes lines at dst_pitch,
 * linesize bytes each (the reference advances 16 bytes per step across lines, :157-168) and refuses an odd `lines`; BORDER refuses border_w > width and
 * 2 * border_h > lines (border.c:158,181-184,203-206); CROP copies out_line_bytes bytes (the reference: req_pitch, crop.c:176-178) and refuses
 * xoff_bytes + out_line_bytes beyond the source's line size.
 * Pitches 0 = the line size (CROP's dst: out_line_bytes), otherwise at least that; the ops work in bytes: any pointer, pitch and stride (LOGO on
 * UG_PF_RG48: multiples of 2); lines 1..65536, at most INT_MAX bytes per frame, frames 1..65535 (grid.z), frame i at src (src2) + i * src_frame_stride ->
 * dst + i * dst_frame_stride, the one overlay on every frame.  Sources and destination must not overlap (LOGO: the overlay and the frame).  An op /
 * format pair without a kernel: UG_HIP_EUNSUPP; anything else: UG_HIP_EINVAL; both before any device call.  Units of 16 bytes at multiples of 16 take
 * the dwordx4 path; bytes of a destination line past the written size keep their content. */
#define UG_CMP_CROP          0
#define UG_CMP_BORDER        1
#define UG_CMP_LOGO          2
#define UG_CMP_INTERLACE     3
#define UG_CMP_INTERLACED_3D 4
#define UG_CMP_SPLIT         5
struct ug_compose_desc {
        const void *src;            /* device (LOGO: NULL or dst) */
        const void *src2;           /* device: INTERLACE's second frame, INTERLACED_3D's second eye; same pitch and stride as src */
        void       *dst;            /* device */
        int         op;             /* UG_CMP_* */
        ug_pixfmt_t format;
        int         width, lines;   /* the source frame (LOGO: the frame), pixels and lines */
        size_t      src_pitch, dst_pitch;
        int         frames;
        size_t      src_frame_stride, dst_frame_stride;
        int         xoff_bytes, yoff, out_line_bytes, out_lines;  /* CROP */
        int         border_w, border_h;                           /* BORDER: pixels, lines */
        unsigned char fill[4];                                    /* BORDER */
        const void *logo;                                         /* LOGO: device, R,G,B,A, logo_w * 4 bytes per line */
        int         logo_w, logo_h, rect_x, rect_y;               /* LOGO: pixels */
        int         grid_x, grid_y;                               /* SPLIT */
        size_t      tile_pitch, tile_stride;                      /* SPLIT: bytes */
};
int ug_hip_compose(const struct ug_compose_desc *d, ug_hip_stream_t stream);
int ug_hip_compose_supported(int op, ug_pixfmt_t format); /* 1 / 0 */
/* crop.c:141-148,170-173 (host): the output size cut down to whole pixel blocks ((int) (w * get_bpp) / block bytes * block bytes, get_bpp a double: 8 / 3
 * for v210, 4.5 for R12L; want 0 = the frame's), the offsets moved back so that the rectangle stays in the frame, x rounded down to whole blocks in
 * bytes.  *out_w can come out 0 (a UYVY crop one pixel wide).  Frame sizes 1..65536, the others 0..65536, else UG_HIP_EINVAL. */
int ug_hip_crop_geometry(ug_pixfmt_t format, int in_w, int in_h, int want_w, int want_h, int xoff, int yoff, int *out_w, int *out_h, int *xoff_bytes,
                         int *yoff_out);
/* logo.c:182-193 (host): rect_x = x, or frame_w - logo_w where x < 0 or x + logo_w > frame_w, then rect_x / bb * bb with bb = get_pf_block_bytes -- a
 * pixel position rounded by the block's BYTE count, C's division toward zero; rect_y the same without the rounding.  A negative result: the frame is
 * left as it is. */
int ug_hip_logo_geometry(ug_pixfmt_t format, int frame_w, int frame_h, int logo_w, int logo_h, int x, int y, int *rect_x, int *rect_y);
/* BORDER's `fill` for a colour R,G,B,A (host): UG_PF_RGB / UG_PF_RGBA the four bytes, UG_PF_UYVY what vc_copylineRGBAtoUYVY makes of two copies of
 * the colour (border.c:161-166). */
int ug_hip_border_pattern(ug_pixfmt_t format, const unsigned char rgba[4], unsigned char out[4]);

/* Pitches of the planar shuffles -- the seven entry points below, ug_hip_from_planar and ug_hip_to_planar: a pitch smaller than the bytes
 * of a line that the conversion reads or writes there is refused (UG_HIP_EINVAL, before any device call, nothing written), on either
 * side: `width` samples for a luma, RGB or 4:4:4 plane, (width + 1) / 2 for a subsampled chroma plane (2 * that for interleaved CbCr;
 * yuv420_to_i420: width / 2), 4 * pairs for a UYVY line (pairs = (width + 1) / 2; width / 2 where only whole pairs are written:
 * yuv422p*_to_uyvy / yuyv), 16 * (width / 6) for yuv422p10le_to_v210's output, 16 * ceil(width / 6) for a v210 source, the tight line
 * for the other packed outputs.  (ug_hip_to_planar walks the source of uyvy_to_nv12 by the reference's 2 * width bytes, two bytes short
 * of a UYVY line at an odd width: by that name odd widths are refused.)
 * Pitch 0 means "tightly packed" only where a comment says so: src_pitch of ug_hip_uyvy_to_i420 / ug_hip_v210_to_p010le and every
 * pitch of the five decode-direction entry points; everywhere else, out_pitch of ug_hip_from_planar included (for every name alike),
 * 0 is a short pitch. */
/* packed -> planar (to_planar.h:53-74); src_pitch 0 = vc_get_linesize(width, UYVY), plane pitches as they are */
int ug_hip_uyvy_to_i420(const void *src_dev, int src_pitch, void *y, int y_pitch, void *u, int u_pitch,
                        void *v, int v_pitch, int width, int height, ug_hip_stream_t stream); /* uyvy_to_i420, to_planar.c:343 */
/* v210_to_p010le (to_planar.c:64-155) for every geometry the reference converts: any width, odd last line (:80-83), the
 * width % 6 margin (:85-89 whole last group on interior line pairs -- written past `width`, and with a pitch shorter than
 * roundup6(width) samples the even line's tail stays on the first samples of the odd line, as in the reference; :139-150 the
 * margin of the last one or two lines copied from two lines above).  src_pitch 0 = vc_get_linesize(width, v210); pitches in
 * bytes.  width % 6 != 0 with fewer than 5 lines -> UG_HIP_EUNSUPP (the reference reads in front of its planes there). */
int ug_hip_v210_to_p010le(const void *src_dev, int src_pitch, void *y, int y_pitch, void *uv, int uv_pitch,
                          int width, int height, ug_hip_stream_t stream);

/* Decode-direction shuffles (from_planar.h:58-77 `struct from_planar_data` flattened to scalars; pitch 0 = tightly packed):
 *   ug_hip_yuv420p_to_uyvy      yuv420p_to_uyvy (from_planar.c:583-683) == i420_8_to_uyvy (video_codec.c:1073-1094) for packed planes
 *   ug_hip_yuv422p_to_uyvy      yuv422p_to_uyvy (from_planar.c:391-423)
 *   ug_hip_yuv422p10le_to_v210  yuv422p10le_to_v210 (from_planar.c:296-333): 16-bit little-endian samples holding 10 bits;
 *                               width / 6 groups per line are written, as in the reference
 *   ug_hip_uyvy_to_i422         uyvy_to_i422 (video_codec.c:949-969), planes passed separately */
int ug_hip_yuv420p_to_uyvy(const void *y_dev, int y_pitch, const void *cb_dev, int cb_pitch, const void *cr_dev, int cr_pitch,
                           void *dst_dev, int dst_pitch, int width, int height, ug_hip_stream_t stream);
int ug_hip_yuv422p_to_uyvy(const void *y_dev, int y_pitch, const void *cb_dev, int cb_pitch, const void *cr_dev, int cr_pitch,
                           void *dst_dev, int dst_pitch, int width, int height, ug_hip_stream_t stream);
int ug_hip_yuv422p10le_to_v210(const void *y_dev, int y_pitch, const void *cb_dev, int cb_pitch, const void *cr_dev, int cr_pitch,
                               void *dst_dev, int dst_pitch, int width, int height, ug_hip_stream_t stream);
int ug_hip_uyvy_to_i422(const void *src_dev, int src_pitch, void *y_dev, int y_pitch, void *cb_dev, int cb_pitch, void *cr_dev,
                        int cr_pitch, int width, int height, ug_hip_stream_t stream);
/* uyvy_to_nv12 (to_planar.c:207-302) as the reference's default (-msse4.1) build computes it: chroma of a line pair is
 * (a + b + 1) >> 1 for the first 16 * (width / 16) pixels (_mm_avg_epu8) and (a + b) / 2 for the scalar tail. */
int ug_hip_uyvy_to_nv12(const void *src_dev, int src_pitch, void *y_dev, int y_pitch, void *cbcr_dev, int cbcr_pitch,
                        int width, int height, ug_hip_stream_t stream);

/* The whole of src/from_planar.h and src/to_planar.h by the reference's own function names (these are the
 * building blocks of libavcodec/{from,to}_lavc_vid_conv.c).  The structs repeat the reference's field for field, all pointers
 * are device pointers:
 *   struct ug_from_planar_data == struct from_planar_data (from_planar.h:58-70); `func` = a decode_planar_func_t name (:86-113):
 *     gbrap_to_rgb gbrap_to_rgba gbrp{10,12,16}le_to_{rgb,rgba,rg48,r10k} gbrp{12,16}le_to_r12l rgbpXX_to_rgb
 *     rgbpXXle_to_{rg48,r10k,r12l} yuv444p_to_vuya yuv420p_to_uyvy yuv420_to_i420 yuv422p_to_uyvy yuv422p_to_yuyv
 *     yuv422pXX_to_uyvy yuv422p10le_to_uyvy yuv422p10le_to_v210
 *   struct ug_to_planar_data == struct to_planar_data (to_planar.h:53-59); `func` = a decode_buffer_func_t name (:65-74):
 *     v210_to_p010le y216_to_p010le uyvy_to_nv12 rgba_to_bgra vuya_to_i444 uyvy_to_i420 r12l_to_gbrp12le r12l_to_gbrp16le
 *     r12l_to_rgbp12le            (the packed source is vc_get_linesize(width, codec) per line, as the reference assumes)
 * Same results as the reference byte for byte, including its habits: no masking of bits above the nominal depth,
 * gbrap_to_rgb[a] striding every plane by in_linesize[0], R12L groups written whole.  Differences, both on the safe side:
 * samples past `width` in the last R12L group are taken as 0 (the reference packs uninitialised stack there), and
 * r12l_to_* writes only the samples inside the picture (the reference writes the whole last group of 8).
 * Unknown name or unusable geometry -> UG_HIP_EINVAL. */
struct ug_from_planar_data {
        int width;
        int height;
        void *out_data;
        unsigned out_pitch;
        const void *in_data[4];
        unsigned in_linesize[4];
        int in_depth;      /* for the XX conversions */
        int log2_chroma_h; /* unused here (the reference needs it for its row-band threading only) */
        int rgb_shift[3];  /* *_to_rgba only */
};
struct ug_to_planar_data {
        int width;
        int height;
        void *out_data[4];
        unsigned out_linesize[4];
        const void *in_data;
};
int ug_hip_from_planar(const char *func, const struct ug_from_planar_data *d, ug_hip_stream_t stream);
int ug_hip_to_planar(const char *func, const struct ug_to_planar_data *d, ug_hip_stream_t stream);
int ug_hip_from_planar_supported(const char *func); /* 1 / 0 */
int ug_hip_to_planar_supported(const char *func);

/* The pixel-format converters of src/libavcodec/to_lavc_vid_conv.c and from_lavc_vid_conv.c -- the work the
 * reference reserves a GPU hook for (to_lavc_vid_conv_cuda.h:55-66 `to_lavc_vid_conv_cuda`, from_lavc_vid_conv_cuda.h:55-66
 * `av_to_uv_convert_cuda`; both return NULL there).  Formats are named as the reference names them: UltraGrid codecs by
 * get_codec_name() ("UYVY", "v210", "RGB", "RGBA", "R10k", ...), frame formats by av_get_pix_fmt_name() ("yuv420p", "yuv422p10le",
 * "nv12", "p010le", "gbrp", "xv30le", ...; FFmpeg's enum values are not used, so nothing here needs its headers).
 * struct ug_av_frame carries the AVFrame fields the reference converters read: data, linesize, width, height, colorspace,
 * color_range (numeric values as in libavutil/pixfmt.h: AVCOL_SPC_BT709 1, BT470BG 5, SMPTE170M 6, SMPTE240M 7; AVCOL_RANGE_JPEG 2).
 *   ug_hip_uv_to_av   to_lavc_vid_conv(): the rows of get_uv_to_av_conversion's table (to_lavc_vid_conv.c:1458-1529) -- sources UYVY, v210, RGB,
 *                     RGBA, Y216, Y416, R10k, R12L, RG48;
 *                     `in_data` is vc_get_linesize(width, codec) per line, `out` holds the (device) planes to fill
 *   ug_hip_av_to_uv   av_to_uv_convert(): the rows of av_to_uv_conversions (from_lavc_vid_conv.c:2049-2172) for software frames (not:
 *                     ayuv64le -> UYVY, y210 -> Y216, hardware frames); YCbCr -> RGB picks BT.601 / BT.709 and limited / full range from the
 *                     frame as get_cs_for_conv does (:2614-2658)
 * Results equal the reference functions' byte for byte, slips included (listed in csrc/lavc_conv.hip).  No row: UG_HIP_EUNSUPP.
 * Like the reference functions, some converters work in whole pixel groups (6 for v210, 8 for R12L, 2 for 4:2:2): they may READ up to one
 * group past the end of the last line of a plane (keep the allocation padded, as FFmpeg does) and they WRITE the whole last group of a line
 * when the line size has room for it -- never past the line size. */
struct ug_av_frame {
        void *data[4];
        int linesize[4];
        int width;
        int height;
        int colorspace;
        int color_range;
};
int ug_hip_uv_to_av(const char *uv_codec, const char *av_pixfmt, const void *in_data_dev, const struct ug_av_frame *out, ug_hip_stream_t stream);
int ug_hip_av_to_uv(const char *av_pixfmt, const char *uv_codec, void *dst_dev, int pitch, const struct ug_av_frame *in, const int rgb_shift[3],
                    ug_hip_stream_t stream);
int ug_hip_uv_to_av_supported(const char *uv_codec, const char *av_pixfmt); /* 1 / 0 */
int ug_hip_av_to_uv_supported(const char *av_pixfmt, const char *uv_codec);
/* get_color_coeffs(cs, depth) (color_space.c:149-184): cs 0 = CS_DFL (= BT.709, the reference's default), 1 = BT.601, 2 = BT.709; depth 0 (full range), 8, 10, 12, 16; out = the 14 fields
 * of struct color_coeffs in declaration order */
int ug_hip_color_coeffs(int cs, int depth, int out[14]);
/* compute_color_coeffs(kr, kb, depth) (color_space.c:193-197): the same 14 fields for arbitrary luma weights (host arithmetic in doubles) */
int ug_hip_compute_color_coeffs(double kr, double kb, int depth, int out[14]);

/* ------------------------------------------------------------------------------------
 * JPEG: 8x8 forward DCT + quantisation (the stage libgpujpeg provides behind
 * gpujpeg_encoder_encode, src/video_compress/gpujpeg.cpp:624)
 * ---------------------------------------------------------------------------------- */
/* Annex-K tables scaled by quality (1..100), natural order; comp 0 luma / 1 chroma */
void ug_hip_jpeg_qtable(int quality, int comp, uint8_t table[64]);
/* fp32 reciprocal divisors (AAN scale folded in), natural order */
void ug_hip_jpeg_divisors(const uint8_t qtable[64], float div[64]);
/* One 8-bit plane -> int16 coefficients, zig-zag order, 64 per block, blocks raster order.
 * blocks_w*8 >= width, blocks_h*8 >= height; edge samples replicated.  `div_dev` = 64 floats
 * in device memory.  coef_dev (may be NULL) receives the unquantised fp32 coefficients. */
int ug_hip_jpeg_fdct_quant_plane(const void *plane_dev, int pitch, int width, int height,
                                 int blocks_w, int blocks_h, const float *div_dev,
                                 int16_t *out_dev, float *coef_dev, ug_hip_stream_t stream);
/* Fused UYVY -> 4:2:0 (uyvy_to_i420 rounding) -> FDCT+quantise of Y, Cb, Cr without the
 * I420 round trip through HBM.  Block counts follow 16x16 MCUs: luma (2*mcu_w) x (2*mcu_h)
 * blocks, chroma mcu_w x mcu_h each, mcu_w = ceil(width/16), mcu_h = ceil(height/16).
 * out_y / out_cb / out_cr as above. div_dev = 128 floats (luma then chroma). */
int ug_hip_uyvy_to_jpeg420_coeffs(const void *src_dev, int src_pitch, int width, int height,
                                  const float *div_dev, int16_t *out_y, int16_t *out_cb,
                                  int16_t *out_cr, ug_hip_stream_t stream);
/* Same for 4:2:2, the sampling UltraGrid's GPUJPEG module selects for UYVY input when no `subsampling=` option is
 * given (gpujpeg.cpp:295-302: autoselect = the input codec's subsampling; UYVY is handed over as GPUJPEG_422_U8_P1020,
 * :339): chroma samples are taken as they are (uyvy_to_i422, video_codec.c:949-969), MCU = 16x8:
 * luma (2*mcu_w) x mcu_h blocks, chroma mcu_w x mcu_h each, mcu_w = ceil(width/16), mcu_h = ceil(height/8). */
int ug_hip_uyvy_to_jpeg422_coeffs(const void *src_dev, int src_pitch, int width, int height,
                                  const float *div_dev, int16_t *out_y, int16_t *out_cb,
                                  int16_t *out_cr, ug_hip_stream_t stream);

/* Both of the above over `frames` images per launch (grid.z = image; tiles of a frame or consecutive frames): image i is read at
 * src + i * src_frame_stride and its planes are written i * luma_frame_stride / i * chroma_frame_stride BYTES after out_y /
 * out_cb, out_cr (multiples of 16).  subsampling = 420 or 422.  A 4K frame is a 13 us launch: batching is what fills the GPU. */
int ug_hip_uyvy_to_jpeg42x_coeffs_batch(int subsampling, const void *src_dev, int src_pitch, int width, int height,
                                        const float *div_dev, int16_t *out_y, int16_t *out_cb, int16_t *out_cr, int frames,
                                        size_t src_frame_stride, size_t luma_frame_stride, size_t chroma_frame_stride,
                                        ug_hip_stream_t stream);

/* Complete baseline JPEG encoder (interleaved scan, restart intervals) = FDCT+quantise as above + Huffman coding (T.81
 * Annex K.3 tables) + headers.  Object shape of gpujpeg_encoder_create / _encode / _destroy
 * (src/video_compress/gpujpeg.cpp:353,624,639).  Sampling / input pairs, as the reference module feeds GPUJPEG
 * (gpujpeg.cpp:227-236,295-305,333-344):
 *   420: UG_PF_UYVY (line pairs averaged, uyvy_to_i420) or UG_PF_I420 (planes back to back, passthrough)   JFIF YCbCr
 *   422: UG_PF_UYVY (samples as they are, uyvy_to_i422)                                                     JFIF YCbCr
 *   420 / 422 with UG_JPEG_INPUT_RGB (create_ex below): UG_PF_RGB, components R (2x2 / 2x1), G, B (1x1)       Adobe R,G,B
 *   444: UG_PF_RGB, components stay R, G, B (color_space_internal = GPUJPEG_RGB); written the libjpeg way for JCS_RGB:
 *        Adobe APP14 transform 0, component ids 'R','G','B', quantiser / Huffman table 0 for every component.
 * `encode` is synchronous on `stream` (it returns the stream length).  ug_hip_jpeg_encoder_max_size() is the capacity that can
 * never overflow (every coefficient at its longest code, every byte stuffed: ~10 B per pixel); a smaller out_capacity is allowed:
 * if the stream does not fit, UG_HIP_EINVAL is returned with *out_len = the size it needs and the buffer contents undefined.
 * restart_interval: MCUs per restart interval, 1..65535; 0 = none (one entropy-coded segment, no DRI -- for readers that cannot take restart markers): a lane per
 * block, bit positions by prefix sum, byte stuffing as a second prefix sum; one more host synchronisation per frame; 0.24 ms per 1080p frame, 0.63 ms at 4K against
 * 0.08 / 0.16 ms with restart intervals (profiles/r06_encode_no_restart.txt). */
typedef struct ug_hip_jpeg_encoder ug_hip_jpeg_encoder;
int    ug_hip_jpeg_encoder_create(int width, int height, int quality, int restart_interval, ug_hip_jpeg_encoder **out);
/* subsampling = 420, 422 or 444 (gpujpeg.cpp:406-408 `subsampling=` option); ug_hip_jpeg_encoder_create() is the 420 form.
 * subsampling = 4444 (GPUJPEG_SUBSAMPLING_4444, what `-c jpeg:alpha` asks of GPUJPEG for RGBA input, gpujpeg.cpp:316-336): R, G, B and alpha,
 * fed UG_PF_RGBA (bytes R, G, B, A) and nothing else -- the R,G,B 4:4:4 stream of the same options with a fourth component 'A' behind (Adobe
 * transform 0, every component 1x1 with quantiser and Huffman table 0; interleaved: an MCU of four blocks; UG_JPEG_NONINTERLEAVED: four scans). */
int    ug_hip_jpeg_encoder_create_sub(int width, int height, int quality, int restart_interval, int subsampling,
                                      ug_hip_jpeg_encoder **out);
/* The rest of the reference module's encoder options (src/video_compress/gpujpeg.cpp:303-305,396-405):
 *   internal_cs  color_space_internal -- the colour space the samples are CODED in.  UG_JPEG_CS_ASIS (what the two calls above do): the samples as
 *                they come -- R, G, B for RGB input, the BT.709 limited-range Y'CbCr of UltraGrid's UYVY / I420 for the rest.  Otherwise the encoder
 *                converts in front of its forward DCT (ug_hip_jpeg_colour_convert below), taking RGB input as full-range R'G'B' and UYVY as BT.709
 *                limited range: RGB input + a Y'CbCr space -> a JFIF-shaped stream, components 1, 2, 3, chroma tables for Cb and Cr (Y601full IS
 *                JFIF); UYVY input + BT.601 (either range) -> the usual 4:2:x stream of the converted samples; UG_JPEG_CS_RGB with RGB input and
 *                UG_JPEG_CS_YCBCR_BT709 with UYVY / I420 input = UG_JPEG_CS_ASIS.  Not offered (UG_HIP_EUNSUPP): R, G, B components with
 *                subsampling 420 / 422 without UG_JPEG_INPUT_RGB, UG_JPEG_INPUT_RGB with a Y'CbCr space, I420 with a conversion
 *                (ug_hip_yuv420p_to_uyvy first, as the module does), a Y'CbCr space or UG_JPEG_INPUT_UYVY with subsampling 4444 (no reader takes Y'CbCr + alpha; UYVY has none).  The colour stage is UNPINNED towards libgpujpeg like the FDCT: published BT.601 /
 *                BT.709 definitions, fp32.
 *   flags        UG_JPEG_NONINTERLEAVED (subsampling 444 / 4444, or 420 / 422 with UG_JPEG_INPUT_RGB): one scan per component (T.81 A.2.2; restart intervals count blocks of the scan's
 *                component) -- the reference's DEFAULT for RGB input (interleaved = 0 unless `:interleaved`, gpujpeg.cpp:303); the header then
 *                carries what those scans use (RGB: quantiser and Huffman table 0 only).  Three coder launches, each going on where the one before
 *                ended (one synchronisation, no intermediate buffer); the single interleaved scan is ONE fused kernel and faster.
 *                UG_JPEG_INPUT_UYVY (subsampling 444 only): the 4:4:4 encoder is fed UYVY instead of RGB (`-c jpeg:subsampling=444` on a 4:2:2
 *                source, gpujpeg.cpp:297-302 with GPUJPEG_422_U8_P1020 input): every pixel takes its pair's chroma, and the samples are coded as
 *                they are (UG_JPEG_CS_ASIS / _BT709: a Y'CbCr stream like the one RGB input + _BT709 gives), converted to BT.601 (either range),
 *                or converted to R, G, B (UG_JPEG_CS_RGB: the R,G,B stream of RGB input, from a 4:2:2 source).
 *                UG_JPEG_INPUT_RGB (subsampling 420 / 422, internal_cs UG_JPEG_CS_ASIS or UG_JPEG_CS_RGB; the mirror of UG_JPEG_INPUT_UYVY): the 4:2:x
 *                encoder is fed UG_PF_RGB (any pitch) and codes R, G, B components -- what the reference asks of GPUJPEG for RGB input with
 *                `subsampling=420|422` (color_space_internal stays GPUJPEG_RGB, gpujpeg.cpp:295-305).  SOF0: 'R' sampled 2x2 (420) / 2x1 (422), 'G' and
 *                'B' 1x1; quantiser and Huffman table 0 for every component, and only table 0 in the header; Adobe APP14 transform 0, no JFIF.
 *                G and B are the box average of their 2x2 / 2x1 pixels, rounded half up, the last column / row taken again where a group runs
 *                past the picture; blocks past a component plane replicate that plane's last sample.  With UG_JPEG_NONINTERLEAVED each scan covers
 *                its component's own ceil(x / 8) x ceil(y / 8) blocks (T.81 A.2.2; the R scan: ceil(width / 8) x ceil(height / 8)), restart
 *                intervals count them, and every scan starts again at RST0.  Encoding UYVY, I420 or RGBA with such an encoder: UG_HIP_EUNSUPP;
 *                UG_JPEG_INPUT_RGB with subsampling 444 / 4444 or with UG_JPEG_INPUT_UYVY: UG_HIP_EINVAL.  The samples (the downsampling) are
 *                UNPINNED towards libgpujpeg, like the FDCT: its preprocessor is not in the reference tree. */
#define UG_JPEG_CS_ASIS                0
#define UG_JPEG_CS_RGB                 1 /* GPUJPEG_RGB: full-range R'G'B' */
#define UG_JPEG_CS_YCBCR_BT601         2 /* GPUJPEG_YCBCR_BT601: limited range (16-235 / 16-240) */
#define UG_JPEG_CS_YCBCR_BT601_256LVLS 3 /* GPUJPEG_YCBCR_BT601_256LVLS: full range -- the JFIF colour space */
#define UG_JPEG_CS_YCBCR_BT709         4 /* GPUJPEG_YCBCR_BT709: limited range */
#define UG_JPEG_NONINTERLEAVED         1
#define UG_JPEG_INPUT_UYVY             2
#define UG_JPEG_INPUT_RGB              4
int    ug_hip_jpeg_encoder_create_ex(int width, int height, int quality, int restart_interval, int subsampling, int internal_cs, int flags,
                                     ug_hip_jpeg_encoder **out);
/* The colour stage by itself.  m[12]: out_i = m[4 i] * in_0 + m[4 i + 1] * in_1 + m[4 i + 2] * in_2 + m[4 i + 3] on 8-bit code values, cs_in -> cs_out
 * (UG_JPEG_CS_RGB .. UG_JPEG_CS_YCBCR_BT709), derived in double from Kr / Kb of BT.601 (0.299, 0.114) and BT.709 (0.2126, 0.0722) and the 219 / 224
 * (limited) or 255 / 255 (256 levels) code ranges.  convert: fmt = UG_PF_RGB (3 bytes per pixel, whatever the three components mean) or UG_PF_UYVY
 * (every pixel with its pair's chroma, the two chroma results of a pair averaged); fp32, one multiply-add at a time, clamp, round to nearest even;
 * pitch 0 = packed. */
int    ug_hip_jpeg_colour_matrix(int cs_in, int cs_out, float m[12]);
int    ug_hip_jpeg_colour_convert(ug_pixfmt_t fmt, int cs_in, int cs_out, const void *src_dev, int src_pitch, void *dst_dev, int dst_pitch, int width, int height,
                                  ug_hip_stream_t stream);
void   ug_hip_jpeg_encoder_destroy(ug_hip_jpeg_encoder *enc);
size_t ug_hip_jpeg_encoder_max_size(const ug_hip_jpeg_encoder *enc);
/* Pitch and alignment of the source (encode and encode_batch alike, whatever kernels the restart interval, the size and the alignment
 * select): src_pitch 0 = packed, else at least the line (UG_PF_UYVY: ug_hip_linesize, UG_PF_RGB 3, UG_PF_RGBA 4 bytes per pixel).
 * UG_PF_UYVY and UG_PF_RGBA are lines of 32-bit words: src_dev, src_pitch and, with frames > 1, src_stride are multiples of 4 (multiples
 * of 16, with a width that is one, take the 128-bit loads).  UG_PF_RGB: any pitch from the line size up and any address.  UG_PF_I420 is
 * tightly packed: src_pitch 0 or the width.  Only the width x height pixels are read as pixels: blocks that reach past the picture repeat
 * its last column / row, never the line padding.  Anything else is UG_HIP_EINVAL, before any device work, and nothing is written. */
int    ug_hip_jpeg_encoder_encode(ug_hip_jpeg_encoder *enc, ug_pixfmt_t in, const void *src_dev, int src_pitch,
                                  void *out_dev, size_t out_capacity, size_t *out_len, ug_hip_stream_t stream);
/* `frames` (1..16) frames of the same geometry in ONE call: one launch sequence over all of them (UYVY / RGB input: ONE kernel does the
 * forward DCT, the quantiser, the Huffman coding and the byte stuffing of every frame, a second small one assembles the streams), one
 * synchronisation, `frames` lengths.  Frame f is read at src_dev + f * src_stride and its stream
 * written at out_dev + f * out_stride (a multiple of 16, >= out_capacity = what one stream may take); out_len[f] = its length; with frames > 1
 * a stream that does not fit is reported per frame -- out_len[f] > out_capacity = the size it needs, the other streams are complete and
 * the call succeeds (the one-frame call returns UG_HIP_EINVAL for it).  Every
 * stream is byte-identical to what ug_hip_jpeg_encoder_encode writes for that frame.  (gpujpeg.cpp:617-631 encodes one frame per
 * call; this is for callers that hold several queued frames: 14 us per 4K 4:2:0 frame at 8 per call against 38 us one by one.) */
int    ug_hip_jpeg_encoder_encode_batch(ug_hip_jpeg_encoder *enc, ug_pixfmt_t in, int frames, const void *src_dev, int src_pitch,
                                        size_t src_stride, void *out_dev, size_t out_stride, size_t out_capacity, size_t *out_len,
                                        ug_hip_stream_t stream);

/* ------------------------------------------------------------------------------------
 * JPEG decoder (receive side: gpujpeg_decoder_create / _decode / _destroy behind
 * src/video_decompress/gpujpeg.c:74-140,292-301)
 * ---------------------------------------------------------------------------------- */
/* Baseline JPEG (8-bit, Huffman; 1 component, 3 components, or 4 at 4:4:4:4, interleaved or one scan per component; restart intervals make the
 * entropy-coded data parallel: one lane per restart segment) -> `out` in device memory.
 * Three-component sampling: factors H, V of 1, 2 or 4, at most 10 blocks in an interleaved MCU, component 0 (Y' or R) at the full resolution,
 * components 1 and 2 with the same factors at a ratio to it of 1x1, 2x1, 2x2, 1x2, 4x1 or 4x2 (read_info: 444, 422, 420, 440, 411, 410),
 * Y'CbCr and R,G,B alike; anything else UG_HIP_EUNSUPP before any device work.  4:4:4 / 4:2:2 / 4:2:0 at their usual factors (luma 1x1, 2x1,
 * 2x2, chroma 1x1) and 4:4:4 R,G,B take the paths below; every other layout one kernel (layout_pack_kernel) by REPLICATION -- a component
 * sample covers its rx x ry pixels, unpinned towards libgpujpeg: R,G,B -> RGB / RGBA packed as below, -> UYVY with vc_copylineRGBtoUYVY's
 * arithmetic on the pixel pair; Y'CbCr -> UYVY with the pair's chroma (a + b) / 2 (4:4:0 is averaged, 4:2:2-like ratios hand their samples
 * back), -> RGB / RGBA through that UYVY; I420 stays for 4:2:0 streams.  Odd widths: the last pair's second pixel is its first.
 *   Per layout:
 *   YCbCr streams -> UG_PF_UYVY (4:2:2: samples as they are; 4:2:0: chroma lines repeated, yuv420p_to_uyvy; 4:4:4: chroma pairs averaged),
 *                    UG_PF_RGB / UG_PF_RGBA (the UYVY form through vc_copylineUYVYtoRGB[A]: BT.709 limited range, as UltraGrid codes it),
 *                    UG_PF_I420 (4:2:0 streams: planes back to back);
 *   R,G,B streams (Adobe APP14 transform 0 or component ids 'R','G','B': what `-c jpeg` writes for RGB input) -> UG_PF_RGB / UG_PF_RGBA
 *                    directly, UG_PF_UYVY through vc_copylineRGBtoUYVY's arithmetic.
 *   R,G,B,A streams (4 components, each 1x1; no Adobe marker or transform 0: what subsampling 4444 writes, and what libjpeg writes for a 4-channel
 *                    image) -> as R,G,B streams; UG_PF_RGBA with the shifts (0, 8, 16) carries the A sample in the top byte (GPUJPEG's
 *                    4444_U8_P0123), other shifts 0xFF there; UG_PF_NONE: plane 3 is A.  Y'CbCr-K (Adobe transform 1 / 2) and subsampled
 *                    four-component streams: UG_HIP_EUNSUPP.
 *   one-component (greyscale) streams: a Y'CbCr picture with both chroma planes at 128, every output above (what another sender's grey MJPEG needs).
 * The component planes equal libjpeg's bit for bit (integer IDCT jidctint).  `jpeg_host` is host memory (compressed frames arrive from the
 * network); everything after the header parse is asynchronous on `stream` (a stream in pinned memory is read by the copy engine when the stream
 * gets there: keep it until then; pageable memory is staged before the call returns; a scan WITHOUT restart intervals -- one segment, decoded by a lane per 1024
 * bits of it with the decoder's states handed from piece to piece until they settle -- synchronises with the host between its launches).  UG_PF_NONE: decode to the internal planes only
 * (ug_hip_jpeg_decoder_plane).  Not a baseline stream / unsupported layout (incl. a second frame header, or a table redefined between
 * the scans of a one-scan-per-component stream): UG_HIP_EUNSUPP.  Damage inside the entropy-coded data is not
 * an error: a segment ends at its first marker, a missing one decodes as an empty one (what a sequential decoder does).  A decoder object
 * holds the work buffers of one frame in flight: one object per thread / per frame in flight.
 * Pitch and alignment of the destination: dst_pitch 0 = packed, else at least the line of `out` (ug_hip_linesize).  UG_PF_UYVY and
 * UG_PF_RGBA from the streams with kernels of their own -- Y'CbCr 4:4:4 / 4:2:2 / 4:2:0 at their usual factors, R,G,B(,A) 4:4:4, greyscale
 * -- leave as 32-bit words: dst_dev and dst_pitch are multiples of 4, for every one of these streams alike.  UG_PF_RGB: any pitch from the
 * line size up and any address, and so every output of the other sampling layouts (layout_pack_kernel picks its store width from the
 * address).  UG_PF_I420 is tightly packed: dst_pitch 0 or the width.  Only the pixels of the picture are written: line padding and whatever
 * follows the last line stay as they were.  Anything else is UG_HIP_EINVAL, after the header parse and before any device work: nothing is
 * written, and the decoder object takes the next call as if this one had not been made. */
typedef struct ug_hip_jpeg_decoder ug_hip_jpeg_decoder;
int  ug_hip_jpeg_decoder_create(ug_hip_jpeg_decoder **out);
void ug_hip_jpeg_decoder_destroy(ug_hip_jpeg_decoder *dec);
/* header only: subsampling = 444 / 422 / 420 / 440 / 411 / 410 (the chroma's ratio to the full resolution, as above) / 400 (greyscale) /
 * 4444 (R, G, B, A; is_rgb = 1); any pointer may be NULL */
int  ug_hip_jpeg_read_info(const void *jpeg_host, size_t len, int *width, int *height, int *subsampling, int *is_rgb, int *restart_interval);
int  ug_hip_jpeg_decoder_decode(ug_hip_jpeg_decoder *dec, const void *jpeg_host, size_t len, ug_pixfmt_t out, void *dst_dev, int dst_pitch,
                                int rshift, int gshift, int bshift, ug_hip_stream_t stream);
/* The same with the picture size the caller sized `dst_dev` for (0 = not checked): a stream whose frame header says otherwise is refused
 * with UG_HIP_EINVAL before anything is written -- streams come from the network, and the size check must not depend on two separate
 * header parses (ug_hip_jpeg_read_info, then this) agreeing. */
int  ug_hip_jpeg_decoder_decode_sized(ug_hip_jpeg_decoder *dec, const void *jpeg_host, size_t len, int expect_width, int expect_height,
                                      ug_pixfmt_t out, void *dst_dev, int dst_pitch, int rshift, int gshift, int bshift, ug_hip_stream_t stream);
/* component plane of the last decode (device memory, padded to whole MCUs; width / height = the component's own size) */
int  ug_hip_jpeg_decoder_plane(const ug_hip_jpeg_decoder *dec, int component, const void **plane_dev, int *pitch, int *width, int *height);

#ifdef __cplusplus
}
#endif
#endif /* UG_MI355X_H */
