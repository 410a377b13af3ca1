/**
 * @file capture_filter_pixel_mi355x.c
 * UltraGrid's per-pixel colour filters and its two mirror filters on an MI355X through libug_mi355x.so (include/ug_mi355x.h:
 * ug_hip_pixel_filter), as capture filters (`-F`) and -- through the reference's own ADD_VO_PP_CAPTURE_FILTER_WRAPPER -- as video postprocessors
 * (`-p`), beside the reference's CPU modules (which exist in every build: no name is taken over):
 *
 *   matrix_mi355x:a:b:c:d:e:f:g:h:i[:no-bound-check]   src/capture_filter/matrix.c     UYVY (comes out as RGB), RGB, RG48; others: NULL
 *   matrix2_mi355x:a:..:i | matrix2_mi355x:y601_to_y709 src/capture_filter/matrix2.c    UYVY, v210, Y416; others: the output frame, unwritten
 *   gamma_mi355x:value[:8|:16]                         src/capture_filter/gamma.cpp    RGB, RG48; others: NULL
 *   grayscale_mi355x                                   src/capture_filter/grayscale.c  UYVY; others: the input frame itself
 *   mirror_mi355x                                      src/capture_filter/mirror.c     UYVY; others: the input frame itself
 *   flip_mi355x                                        src/capture_filter/flip.c       every codec (those without a kernel: line copies on the host)
 *
 * Options are parsed as the reference's parsers parse them: `help` or (matrix, matrix2, gamma) an empty string prints the usage and returns 1;
 * matrix's tenth token is `no-bound-check` as matrix.c:95 spells it (its help text says no-bounds-check; anything else there is an "excess
 * initializer" and ignored with a warning); a number that does not convert only warns; fewer than nine numbers: -1; gamma's depth must be 8 or
 * 16; grayscale, mirror and flip take no option (-1).  One deviation: gamma <= 0 or not finite is refused (-1) where the reference warns and
 * builds tables from inf (include/ug_mi355x.h: ug_hip_gamma_lut).
 * filter(in): the frame goes through a pinned host buffer to the device, ONE launch, and comes back into a new frame (its data malloc'ed, or
 * the postprocessor wrapper's buffer); the state's stream is synchronised before filter returns, also on failure.  Every element is
 * transformed: the reference's gamma leaves the last data_len / element % hardware_concurrency() elements unwritten (gamma.cpp:133-138).
 * A size or codec change between frames needs nothing from the caller: the buffers follow the frame.  The GPU: --param mi355x-device / -D
 * (mi355x_receiver.h); the states of this process take the listed devices in turn.
 */
#include <errno.h>
#include <math.h>
#include <stdbool.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#ifdef HAVE_CONFIG_H
#include "config.h"
#endif
#include "capture_filter.h"
#include "compat/c23.h"
#include "debug.h"
#include "lib_common.h"
#include "types.h"
#include "utils/macros.h"
#include "video_codec.h"
#include "video_frame.h"
#include "vo_postprocess/capture_filter_wrapper.h"

#include "mi355x_gpu_state.h"
#include "ug_codec_map.h"

#define MOD_NAME "[pixel filter MI355X] "

enum pxf_kind { K_MATRIX, K_MATRIX2, K_GAMMA, K_GRAYSCALE, K_MIRROR, K_FLIP };
static const char *const kind_names[] = { "matrix_mi355x", "matrix2_mi355x", "gamma_mi355x", "grayscale_mi355x", "mirror_mi355x", "flip_mi355x" };

enum { LUT8_OFF = 0, LUT8_16_OFF = 256, LUT16_8_OFF = 256 + 512, LUT16_OFF = 256 + 512 + 65536, LUTS_LEN = 256 + 512 + 65536 + 131072 };

struct state_pxf_mi355x {
        enum pxf_kind   kind;
        double          matrix[9];
        bool            check_bounds;
        int             out_depth;        ///< gamma: 0, 8 or 16 (0 means keep)
        unsigned char  *luts;             ///< gamma: the four host tables back to back (8->8, 8->16, 16->8, 16->16)
        struct mi355x_buf luts_dev;
        void           *vo_pp_out_buffer; ///< buffer to write to if we use vo_pp wrapper (otherwise unused)
        struct mi355x_gpu gpu;
        struct mi355x_buf host_in, dev_in, dev_out; ///< host_in: pinned
};

static unsigned pxf_mi355x_state_count; // the states of this process take the listed devices in turn

static void usage(enum pxf_kind kind)
{
        switch (kind) {
        case K_MATRIX:
                printf("Matrix transformation of the pixels on the MI355X (UYVY -> RGB, RGB, RG48):\n\t-F/-p matrix_mi355x:a:b:c:d:e:f:g:h:i[:no-bound-check]\n");
                break;
        case K_MATRIX2:
                printf("Matrix transformation of Y Cb Cr on the MI355X (UYVY, v210, Y416):\n\t-F/-p matrix2_mi355x:a:b:c:d:e:f:g:h:i\n\t-F/-p matrix2_mi355x:y601_to_y709\n");
                break;
        case K_GAMMA:
                printf("Gamma transformation on the MI355X (RGB, RG48):\n\t-F/-p gamma_mi355x:value[:8|:16]\n");
                break;
        default:
                printf("%s takes no arguments (grayscale / horizontal mirror of UYVY, vertical flip of anything) -- on the MI355X\n", kind_names[kind]);
                break;
        }
}

/// nine numbers as matrix.c:93-116 and matrix2.c:112-134 read them; @returns how many were read
static int parse_matrix(struct state_pxf_mi355x *s, const char *cfg)
{
        char *cfg_c = strdup(cfg), *save_ptr = NULL, *item = NULL, *tmp = cfg_c;
        int i = 0;
        while ((item = strtok_r(tmp, ":", &save_ptr)) != NULL) {
                if (s->kind == K_MATRIX2 && i == 0 && strcmp(item, "y601_to_y709") == 0) {
                        ug_hip_matrix2_preset(item, s->matrix);
                        i = 9;
                        break;
                }
                if (i == 9) {
                        if (s->kind == K_MATRIX && strcmp(item, "no-bound-check") == 0) {
                                s->check_bounds = false;
                        } else if (s->kind == K_MATRIX) {
                                MSG(WARNING, "Excess initializer given: %s\n", item);
                        }
                        break; // (matrix2 writes a tenth number past its array; not reproduced)
                }
                char *endptr = NULL;
                errno = 0;
                s->matrix[i++] = strtod(item, &endptr);
                if (errno != 0 || *endptr != '\0') {
                        MSG(WARNING, "Problem converting number %s\n", item);
                }
                tmp = NULL;
        }
        free(cfg_c);
        return i;
}

static void done(void *state)
{
        struct state_pxf_mi355x *s = state;
        mi355x_gpu_close(&s->gpu); // (nothing on a state whose stream was never made: its bufs are empty.  The device stays the current one)
        mi355x_buf_release(&s->host_in);
        mi355x_buf_release(&s->dev_in);
        mi355x_buf_release(&s->dev_out);
        mi355x_buf_release(&s->luts_dev);
        free(s->luts);
        free(s);
}

static int init_common(enum pxf_kind kind, const char *cfg, void **state)
{
        const bool takes_options = kind == K_MATRIX || kind == K_MATRIX2 || kind == K_GAMMA;
        if (takes_options ? (strlen(cfg) == 0 || strcmp(cfg, "help") == 0) : strlen(cfg) > 0) {
                usage(kind);
                return takes_options || strcmp(cfg, "help") == 0 ? 1 : -1;
        }
        struct state_pxf_mi355x *s = calloc(1, sizeof *s);
        if (s == NULL) {
                return -1;
        }
        s->kind = kind;
        s->check_bounds = true;
        if (kind == K_MATRIX || kind == K_MATRIX2) {
                const int n = parse_matrix(s, cfg);
                if (n != 9) {
                        MSG(ERROR, "Not enough numbers for transformation matrix - expected: 9, got: %d\n", n);
                        free(s);
                        return -1;
                }
        } else if (kind == K_GAMMA) { // gamma.cpp:166-183
                char *endptr = NULL;
                errno = 0;
                const double gamma = strtod(cfg, &endptr);
                if (errno != 0 || (*endptr != '\0' && *endptr != ':')) {
                        MSG(WARNING, "Using gamma value %g\n", gamma);
                }
                long bits = 0;
                if (*endptr != '\0') {
                        endptr += 1;
                        bits = strtol(endptr, &endptr, 0);
                        if ((bits != 8 && bits != 16) || *endptr != '\0') {
                                MSG(ERROR, "Wrong number of bits (only 8 or 16)!\n");
                                free(s);
                                return -1;
                        }
                }
                s->out_depth = (int) bits;
                s->luts = malloc(LUTS_LEN);
                if (s->luts == NULL || ug_hip_gamma_lut(gamma, 8, 8, s->luts + LUT8_OFF) != UG_HIP_SUCCESS ||
                    ug_hip_gamma_lut(gamma, 8, 16, s->luts + LUT8_16_OFF) != UG_HIP_SUCCESS || ug_hip_gamma_lut(gamma, 16, 8, s->luts + LUT16_8_OFF) != UG_HIP_SUCCESS ||
                    ug_hip_gamma_lut(gamma, 16, 16, s->luts + LUT16_OFF) != UG_HIP_SUCCESS) {
                        MSG(ERROR, "gamma %g: a finite value above 0 is needed\n", gamma);
                        free(s->luts);
                        free(s);
                        return -1;
                }
        }
        s->host_in.pinned = true;
        if (!mi355x_gpu_open(&s->gpu, &pxf_mi355x_state_count, MOD_NAME)) {
                done(s);
                return -1;
        }
        *state = s;
        return 0;
}

/// the buffers follow the frame: at least in_len / out_len bytes
static bool reserve(struct state_pxf_mi355x *s, size_t in_len, size_t out_len)
{
        bool ok = mi355x_buf_reserve(&s->host_in, in_len) && mi355x_buf_reserve(&s->dev_in, in_len) && mi355x_buf_reserve(&s->dev_out, out_len);
        if (ok && s->kind == K_GAMMA && s->luts_dev.ptr == NULL) {
                ok = mi355x_buf_reserve(&s->luts_dev, LUTS_LEN) && ug_hip_memcpy(s->luts_dev.ptr, s->luts, LUTS_LEN, UG_HIP_MEMCPY_HOST_TO_DEVICE) == UG_HIP_SUCCESS;
        }
        if (!ok) MSG(ERROR, "cannot allocate the frame buffers: %s\n", ug_hip_last_error_string());
        return ok;
}

static bool run_gpu(struct state_pxf_mi355x *s, const struct video_frame *in, struct video_frame *out)
{
        static const int ops[] = { UG_PXF_MATRIX, UG_PXF_MATRIX2, UG_PXF_LUT, UG_PXF_GRAY, UG_PXF_MIRROR, UG_PXF_FLIP };
        const size_t in_line = (size_t) vc_get_linesize(in->tiles[0].width, in->color_spec), out_line = (size_t) vc_get_linesize(out->tiles[0].width, out->color_spec);
        const size_t rows = in->tiles[0].height, in_len = in_line * rows, out_len = out_line * rows;
        if (in->tiles[0].data_len < in_len || out->tiles[0].data_len < out_len) {
                MSG(ERROR, "frame shorter than %zu lines of %zu bytes\n", rows, in_line);
                return false;
        }
        if (!mi355x_gpu_enter(&s->gpu) || !reserve(s, in_len, out_len)) {
                return false;
        }
        struct ug_pixel_filter_desc d = {
                .src = s->dev_in.ptr, .dst = s->dev_out.ptr, .op = ops[s->kind], .format = ug_pixfmt_from_codec(in->color_spec),
                .out_format = ug_pixfmt_from_codec(out->color_spec), .width = (int) in->tiles[0].width, .lines = (int) rows, .frames = 1,
                .clamp = s->check_bounds,
        };
        memcpy(d.matrix, s->matrix, sizeof d.matrix);
        if (s->kind == K_GAMMA) {
                const bool in16 = in->color_spec == RG48, out16 = out->color_spec == RG48;
                d.lut_dev = (char *) s->luts_dev.ptr + (in16 ? (out16 ? LUT16_OFF : LUT16_8_OFF) : (out16 ? LUT8_16_OFF : LUT8_OFF));
        }
        memcpy(s->host_in.ptr, in->tiles[0].data, in_len);
        const bool ok = ug_hip_upload_ordered_ex(s->gpu.device, s->dev_in.ptr, s->host_in.ptr, in_len, UG_HIP_MEMCPY_HOST_TO_DEVICE, s->gpu.stream, 0) == UG_HIP_SUCCESS &&
                        ug_hip_pixel_filter(&d, s->gpu.stream) == UG_HIP_SUCCESS &&
                        ug_hip_download_2d_ordered_ex(s->gpu.device, out->tiles[0].data, out_line, s->dev_out.ptr, out_line, out_line, rows, s->gpu.stream, 0) == UG_HIP_SUCCESS;
        return mi355x_gpu_finish(&s->gpu, ok, kind_names[s->kind]);
}

static struct video_frame *filter(void *state, struct video_frame *in)
{
        if (in == nullptr) {
                return nullptr;
        }
        struct state_pxf_mi355x *s = state;
        const codec_t c = in->color_spec;
        struct video_desc desc = video_desc_from_frame(in);
        bool supported = true;
        switch (s->kind) {
        case K_MATRIX:
                if (c != UYVY && c != RGB && c != RG48) {
                        MSG(ERROR, "Only UYVY, RGB or RG48 is currently supported!\n");
                        VIDEO_FRAME_DISPOSE(in);
                        return NULL;
                }
                if (c == UYVY) desc.color_spec = RGB;
                break;
        case K_MATRIX2:
                supported = c == UYVY || c == v210 || c == Y416;
                break;
        case K_GAMMA:
                if (c != RGB && c != RG48) {
                        MSG(ERROR, "Unable to apply lut on: %s\n", get_codec_name(c));
                        VIDEO_FRAME_DISPOSE(in);
                        return NULL;
                }
                if (s->out_depth != 0) desc.color_spec = s->out_depth == 8 ? RGB : RG48;
                break;
        case K_GRAYSCALE:
        case K_MIRROR:
                if (c != UYVY) {
                        MSG(WARNING, "%s takes UYVY only!\n", kind_names[s->kind]);
                        return in;
                }
                break;
        case K_FLIP:
                break;
        }
        struct video_frame *out = vf_alloc_desc(desc);
        if (s->vo_pp_out_buffer) {
                out->tiles[0].data = s->vo_pp_out_buffer;
        } else {
                out->tiles[0].data = malloc(out->tiles[0].data_len);
                out->callbacks.data_deleter = vf_data_deleter;
        }
        out->callbacks.dispose = vf_free;
        if (!supported) { // matrix2.c:265-273: the frame as allocated
                MSG(ERROR, "Sorry, only UYVY, v210 and Y416 are supported by now (have %s).\n", get_codec_name(c));
                VIDEO_FRAME_DISPOSE(in);
                return out;
        }
        bool ok = true;
        if (s->kind == K_FLIP && ug_hip_pixel_filter_supported(UG_PXF_FLIP, ug_pixfmt_from_codec(c)) != 1) { // flip.c:96-99 on the host
                const size_t linesize = (size_t) vc_get_linesize(in->tiles[0].width, c), h = in->tiles[0].height;
                for (size_t y = 0; y < h; ++y) memcpy(out->tiles[0].data + (h - y - 1) * linesize, in->tiles[0].data + y * linesize, linesize);
        } else {
                ok = run_gpu(s, in, out);
        }
        VIDEO_FRAME_DISPOSE(in);
        if (!ok) {
                if (!s->vo_pp_out_buffer) free(out->tiles[0].data);
                out->callbacks.data_deleter = NULL;
                vf_free(out);
                return NULL;
        }
        return out;
}

static void vo_pp_set_out_buffer(void *state, char *buffer)
{
        struct state_pxf_mi355x *s = state;
        s->vo_pp_out_buffer = buffer;
}

#define PXF_MODULE(name, kind)                                                                                                                  \
        static int init_##name(struct module *parent, const char *cfg, void **state) { (void) parent; return init_common(kind, cfg, state); }    \
        static const struct capture_filter_info capture_filter_##name = { .init = init_##name, .done = done, .filter = filter };                 \
        REGISTER_MODULE(name, &capture_filter_##name, LIBRARY_CLASS_CAPTURE_FILTER, CAPTURE_FILTER_ABI_VERSION);                                 \
        ADD_VO_PP_CAPTURE_FILTER_WRAPPER(name, init_##name, filter, done, vo_pp_set_out_buffer, NULL)

PXF_MODULE(matrix_mi355x, K_MATRIX)
PXF_MODULE(matrix2_mi355x, K_MATRIX2)
PXF_MODULE(gamma_mi355x, K_GAMMA)
PXF_MODULE(grayscale_mi355x, K_GRAYSCALE)
PXF_MODULE(mirror_mi355x, K_MIRROR)
PXF_MODULE(flip_mi355x, K_FLIP)
