/**
 * @file vo_pp_compose_mi355x.c
 * UltraGrid's geometric / compositing filters on an MI355X through libug_mi355x.so (include/ug_mi355x.h: ug_hip_compose), beside the reference's
 * CPU modules (which exist in every build: no name is taken over):
 *
 *   crop_mi355x[:size=<w>x<h>][:width=][:height=][:xoff=][:yoff=]   src/vo_postprocess/crop.c           -p and --capture-filter
 *   border_mi355x[:color=rrggbb][:width=<x>][:height=<y>]           src/vo_postprocess/border.c         -p   (UYVY, RGB, RGBA; others: false)
 *   interlace_mi355x                                                src/vo_postprocess/interlace.c      -p and, through capture_filter/vo_pp_wrapper.h, --capture-filter
 *   interlaced_3d_mi355x                                            src/vo_postprocess/3d-interlaced.c  -p, 2 tiles in, 1 out
 *   split_mi355x:<X>:<Y>                                            src/vo_postprocess/split.c          -p, VO_PP_DOES_CHANGE_TILING_MODE
 *   logo_mi355x:<file.pam>[:<x>[:<y>]]                              src/capture_filter/logo.c           --capture-filter (UYVY, RGB, RGBA, RG48; others: the frame as it is)
 *
 * Options are parsed as the reference's parsers parse them -- border's colour from its second digit on (border.c:90-95), width and height
 * rounded up to even; logo reads its .pam through the reference's pam_read and expands three channels to four (logo.c:92-96); the overlay is
 * uploaded once, at init.  get_out_desc answers as the reference's: crop the cut width, interlace fps / 2 and INTERLACED_MERGED, split the tile
 * count.  interlace answers false for the first frame of each pair.
 * A frame goes through a pinned host buffer to the device, ONE launch, and comes back at the pitch the caller asked for; logo moves only the
 * lines its rectangle covers.  The state's stream is synchronised before a call returns, also on failure.
 * Where the reference leaves its buffers (include/ug_mi355x.h "Deviations") the call fails instead: false from border (a band that does not
 * fit) and interlaced_3d (an odd height, refused at reconfigure); logo leaves the frame as it is for a rectangle that leaves the frame.  crop
 * copies the bytes of the output's line that the source line holds.  The GPU: --param mi355x-device / -D (mi355x_receiver.h).
 */
#include <assert.h>
#include <stdbool.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>

#ifdef HAVE_CONFIG_H
#include "config.h"
#endif
#include "capture_filter.h"
#include "capture_filter/vo_pp_wrapper.h"
#include "compat/c23.h"
#include "debug.h"
#include "lib_common.h"
#include "pixfmt_conv.h"
#include "types.h"
#include "utils/macros.h"
#include "utils/pam.h"
#include "video_codec.h"
#include "video_display.h"
#include "video_frame.h"
#include "vo_postprocess.h"

#include "mi355x_gpu_state.h"
#include "ug_codec_map.h"

#define MOD_NAME "[compose MI355X] "

enum cmp_kind { K_CROP, K_BORDER, K_INTERLACE, K_3D, K_SPLIT, K_LOGO };
static const char *const kind_names[] = { "crop_mi355x", "border_mi355x", "interlace_mi355x", "interlaced_3d_mi355x", "split_mi355x", "logo_mi355x" };

struct state_cmp_mi355x {
        enum cmp_kind   kind;
        int             width, height, xoff, yoff;   ///< crop
        unsigned char   color[4];                    ///< border
        unsigned        bw, bh;
        int             gx, gy;                      ///< split
        unsigned char  *logo;                        ///< logo: R,G,B,A on the host
        unsigned        lw, lh;
        int             x, y;
        struct mi355x_buf logo_dev;
        struct video_desc in_desc, out_desc;         ///< crop: out_desc; all: in_desc of the last reconfigure
        struct video_frame *in[2];                   ///< the frame(s) getf hands out (interlace: odd, even)
        int             last;                        ///< interlace: 0 = odd, 1 = even (interlace.c:56-59)
        struct mi355x_gpu gpu;
        struct mi355x_buf host, dev_in[2], dev_out;  ///< host: pinned
};

static unsigned cmp_mi355x_state_count; // the states of this process take the listed devices in turn

static void done(void *state)
{
        struct state_cmp_mi355x *s = state;
        mi355x_gpu_close(&s->gpu); // (nothing on a state whose stream was never made: its bufs are empty.  The device stays the current one)
        mi355x_buf_release(&s->host);
        mi355x_buf_release(&s->dev_in[0]);
        mi355x_buf_release(&s->dev_in[1]);
        mi355x_buf_release(&s->dev_out);
        mi355x_buf_release(&s->logo_dev);
        vf_free(s->in[0]);
        vf_free(s->in[1]);
        free(s->logo);
        free(s);
}

/// logo.c:72-107
static bool load_logo(struct state_cmp_mi355x *s, const char *filename)
{
        if (strcasecmp(filename + (MAX(strlen(filename), 4) - 4), ".pam") != 0) {
                MSG(ERROR, "Only logo in PAM format is currently supported.\n");
                return false;
        }
        unsigned char *data = NULL;
        struct pam_metadata info;
        if (!pam_read(filename, &info, &data, malloc)) {
                return false;
        }
        s->lw = info.width;
        s->lh = info.height;
        if ((info.ch_count != 3 && info.ch_count != 4) || s->lw < 1 || s->lh < 1) {
                MSG(ERROR, "Unsupported channel count %d in PAM file.\n", info.ch_count);
                free(data);
                return false;
        }
        if (info.ch_count == 3) {
                const int datalen = 4 * (int) s->lw * (int) s->lh;
                unsigned char *tmp = malloc((size_t) datalen);
                vc_copylineRGBtoRGBA(tmp, data, datalen, 0, 8, 16);
                free(data);
                data = tmp;
        }
        s->logo = data;
        return true;
}

static void *init_common(enum cmp_kind kind, const char *config)
{
        if (strcmp(config, "help") == 0 || (kind == K_LOGO && strlen(config) == 0)) {
                printf("%s: the reference's %.*s on the MI355X, the same options\n", kind_names[kind], (int) (strlen(kind_names[kind]) - strlen("_mi355x")), kind_names[kind]);
                return kind == K_INTERLACE || kind == K_3D ? INIT_NOERR : NULL;
        }
        if (kind == K_3D && strlen(config) > 0) {
                printf("3d-interlaced takes no parameters.\n");
                return NULL;
        }
        struct state_cmp_mi355x *s = calloc(1, sizeof *s);
        if (s == NULL) {
                return NULL;
        }
        s->kind = kind;
        s->host.pinned = true;
        s->last = 1;
        s->x = s->y = -1;
        s->bw = s->bh = 10;
        memcpy(s->color, ((uint8_t[]){ 0xff, 0xff, 0x00, 0xff }), sizeof s->color);
        char *tmp = strdup(config), *cfg = tmp, *item = NULL, *save_ptr = NULL;
        bool ok = true;
        int n = 0;
        while (ok && kind != K_INTERLACE && (item = strtok_r(cfg, ":", &save_ptr)) != NULL) {
                cfg = NULL;
                if (kind == K_CROP) { // crop.c:98-124
                        if (strstr(item, "size=") == item) {
                                if (strchr(item, 'x') == NULL) {
                                        MSG(ERROR, "Missing height!\n");
                                        ok = false;
                                } else {
                                        s->width = atoi(strchr(item, '=') + 1);
                                        s->height = atoi(strchr(item, 'x') + 1);
                                }
                        } else if (strncasecmp(item, "width=", strlen("width=")) == 0) {
                                s->width = atoi(item + strlen("width="));
                        } else if (strncasecmp(item, "height=", strlen("height=")) == 0) {
                                s->height = atoi(item + strlen("height="));
                        } else if (strncasecmp(item, "xoff=", strlen("xoff=")) == 0) {
                                s->xoff = atoi(item + strlen("xoff="));
                        } else if (strncasecmp(item, "yoff=", strlen("yoff=")) == 0) {
                                s->yoff = atoi(item + strlen("yoff="));
                        } else {
                                MSG(ERROR, "Wrong config: %s!\n", item);
                                ok = false;
                        }
                } else if (kind == K_BORDER) { // border.c:87-125
                        if (strncasecmp(item, "color=", strlen("color=")) == 0) {
                                const char *color = item + strlen("color=");
                                if (color[0] == '#') {
                                        color += 1;
                                }
                                if (strlen(color) == 6) {
                                        char color_str[3] = "";
                                        color += 1; // (the reference skips a '#' a second time: the colour is read from its second digit on)
                                        for (int i = 0; i < 3; ++i) {
                                                color_str[0] = color[0];
                                                color_str[1] = color[0] != '\0' ? color[1] : '\0';
                                                s->color[i] = (unsigned char) strtol(color_str, NULL, 16);
                                                color += color[0] != '\0' && color[1] != '\0' ? 2 : (color[0] != '\0' ? 1 : 0);
                                        }
                                } else {
                                        MSG(ERROR, "Wrong color format!\n");
                                        ok = false;
                                }
                        } else if (strncasecmp(item, "width=", strlen("width=")) == 0) {
                                s->bw = ((unsigned) atoi(item + strlen("width=")) + 1) / 2 * 2;
                        } else if (strncasecmp(item, "height=", strlen("height=")) == 0) {
                                s->bh = ((unsigned) atoi(item + strlen("height=")) + 1) / 2 * 2;
                        } else {
                                MSG(ERROR, "Wrong config!\n");
                                ok = false;
                        }
                } else if (kind == K_SPLIT) { // split.c:101-114
                        if (n == 0) s->gx = atoi(item);
                        if (n == 1) s->gy = atoi(item);
                } else if (kind == K_LOGO) { // logo.c:127-141
                        if (n == 0) ok = load_logo(s, item);
                        if (n == 1) s->x = atoi(item);
                        if (n == 2) s->y = atoi(item);
                }
                n++;
        }
        free(tmp);
        if (ok && kind == K_SPLIT && (n < 2 || s->gx < 1 || s->gy < 1)) {
                MSG(ERROR, "Wrong usage!\nusage:\n-p split_mi355x:<X>:<Y>\n");
                ok = false;
        }
        if (ok && kind == K_LOGO && s->logo == NULL) {
                fprintf(stderr, "File name with logo required!\n");
                ok = false;
        }
        ok = ok && mi355x_gpu_open(&s->gpu, &cmp_mi355x_state_count, MOD_NAME);
        if (ok && kind == K_LOGO) {
                const size_t len = (size_t) 4 * s->lw * s->lh;
                ok = mi355x_buf_reserve(&s->logo_dev, len) && ug_hip_memcpy(s->logo_dev.ptr, s->logo, len, UG_HIP_MEMCPY_HOST_TO_DEVICE) == UG_HIP_SUCCESS;
                if (!ok) MSG(ERROR, "cannot upload the logo: %s\n", ug_hip_last_error_string());
        }
        if (!ok) {
                done(s);
                return NULL;
        }
        return s;
}

static bool reconfigure(void *state, struct video_desc desc)
{
        struct state_cmp_mi355x *s = state;
        vf_free(s->in[0]);
        vf_free(s->in[1]);
        s->in[0] = s->in[1] = NULL;
        s->in_desc = desc;
        s->out_desc = desc;
        s->last = 1;
        if (s->kind == K_3D && (desc.tile_count != 2 || desc.height % 2 != 0)) {
                MSG(ERROR, "interlaced_3d_mi355x needs two tiles of an even height (have %u of %u lines)\n", desc.tile_count, desc.height);
                return false;
        }
        if (s->kind == K_SPLIT && (desc.width % (unsigned) s->gx != 0 || desc.height % (unsigned) s->gy != 0)) {
                MSG(ERROR, "split_mi355x: %dx%d tiles do not divide %ux%u\n", s->gx, s->gy, desc.width, desc.height);
                return false;
        }
        if (s->kind == K_CROP) { // crop.c:140-148
                int w = 0, h = 0, xb = 0, yo = 0;
                if (ug_hip_crop_geometry(ug_pixfmt_from_codec(desc.color_spec), (int) desc.width, (int) desc.height, s->width, s->height, s->xoff, s->yoff, &w, &h, &xb,
                                         &yo) != UG_HIP_SUCCESS) {
                        MSG(ERROR, "crop_mi355x: %s\n", ug_hip_last_error_string());
                        return false;
                }
                s->out_desc.width = (unsigned) w;
                s->out_desc.height = (unsigned) h;
        }
        s->in[0] = vf_alloc_desc_data(desc);
        if (s->kind == K_INTERLACE) s->in[1] = vf_alloc_desc_data(desc);
        return true;
}

static struct video_frame *getf(void *state)
{
        struct state_cmp_mi355x *s = state;
        if (s->kind != K_INTERLACE) {
                return s->in[0];
        }
        s->last = (s->last + 1) % 2; // interlace.c:125-139
        return s->in[s->last];
}

static void get_out_desc(void *state, struct video_desc *out, int *in_display_mode)
{
        struct state_cmp_mi355x *s = state;
        *out = s->kind == K_CROP ? s->out_desc : s->in_desc;
        switch (s->kind) {
        case K_CROP:
        case K_BORDER:
                *in_display_mode = DISPLAY_PROPERTY_VIDEO_MERGED;
                break;
        case K_INTERLACE: // (the reference leaves the display mode alone)
                out->interlacing = INTERLACED_MERGED;
                out->fps = s->in_desc.fps / 2.0;
                break;
        case K_3D:
                out->tile_count = 1;
                *in_display_mode = DISPLAY_PROPERTY_VIDEO_SEPARATE_TILES;
                break;
        case K_SPLIT:
                out->width = s->in_desc.width / (unsigned) s->gx;
                out->height = s->in_desc.height / (unsigned) s->gy;
                out->tile_count = (unsigned) (s->gx * s->gy);
                *in_display_mode = DISPLAY_PROPERTY_VIDEO_MERGED;
                break;
        default: break;
        }
}

static bool get_property(void *state, int property, void *val, size_t *len)
{
        (void) state, (void) property, (void) val, (void) len;
        return false;
}

static bool split_get_property(void *state, int property, void *val, size_t *len)
{
        (void) state;
        if (property == VO_PP_DOES_CHANGE_TILING_MODE) { // split.c:63-78
                if (*len >= sizeof(bool)) {
                        *(bool *) val = true;
                        *len = sizeof(bool);
                } else {
                        *len = 0;
                }
                return true;
        }
        return false;
}

/// the buffers follow the frame: a pinned buffer of host_len, device inputs of in_len each, an output of out_len
static bool reserve(struct state_cmp_mi355x *s, size_t host_len, size_t in_len, int inputs, size_t out_len)
{
        bool ok = mi355x_buf_reserve(&s->host, host_len);
        for (int i = 0; ok && i < inputs; i++) ok = mi355x_buf_reserve(&s->dev_in[i], in_len);
        ok = ok && mi355x_buf_reserve(&s->dev_out, out_len);
        if (!ok) MSG(ERROR, "cannot allocate the frame buffers: %s\n", ug_hip_last_error_string());
        return ok;
}

static bool postprocess(void *state, struct video_frame *in, struct video_frame *out, int req_pitch)
{
        static const int ops[] = { UG_CMP_CROP, UG_CMP_BORDER, UG_CMP_INTERLACE, UG_CMP_INTERLACED_3D, UG_CMP_SPLIT, UG_CMP_LOGO };
        struct state_cmp_mi355x *s = state;
        if (in == nullptr) {
                return false;
        }
        if (s->kind == K_INTERLACE) {
                if (in != s->in[0] && in != s->in[1]) { // a capture filter's frame: into the frame getf would have handed out (interlace.c:146-157)
                        struct video_frame *buf = getf(s);
                        for (unsigned t = 0; t < buf->tile_count; ++t) memcpy(buf->tiles[t].data, in->tiles[t].data, MIN(in->tiles[t].data_len, buf->tiles[t].data_len));
                }
                if (s->last == 0) {
                        return false;
                }
        }
        const codec_t c = s->in_desc.color_spec;
        const ug_pixfmt_t fmt = ug_pixfmt_from_codec(c);
        if (ug_hip_compose_supported(ops[s->kind], fmt) != 1) {
                MSG(WARNING, "Unsupported pixel format!\n");
                return false;
        }
        const int w = (int) s->in_desc.width, h = (int) s->in_desc.height;
        const size_t L = (size_t) vc_get_linesize(s->in_desc.width, c), in_len = L * (size_t) h;
        const int inputs = s->kind == K_INTERLACE || s->kind == K_3D ? 2 : 1;
        struct ug_compose_desc d = { .op = ops[s->kind], .format = fmt, .width = w, .lines = h, .frames = 1 };
        size_t lb = L, rows = (size_t) h, out_pitch = L; // bytes and lines of one output tile on the device, their pitch there
        unsigned out_tiles = 1;
        switch (s->kind) {
        case K_CROP: {
                int ow = 0, oh = 0;
                if (ug_hip_crop_geometry(fmt, w, h, s->width, s->height, s->xoff, s->yoff, &ow, &oh, &d.xoff_bytes, &d.yoff) != UG_HIP_SUCCESS || ow < 1) {
                        MSG(ERROR, "crop_mi355x: nothing left of %dx%d\n", w, h);
                        return false;
                }
                lb = MIN((size_t) vc_get_linesize((unsigned) ow, c), L - (size_t) d.xoff_bytes);
                rows = (size_t) oh;
                d.out_line_bytes = (int) lb, d.out_lines = oh;
                out_pitch = lb;
                break;
        }
        case K_BORDER:
                d.border_w = (int) s->bw, d.border_h = (int) s->bh;
                ug_hip_border_pattern(fmt, s->color, d.fill);
                break;
        case K_SPLIT: {
                const unsigned tw = s->in_desc.width / (unsigned) s->gx;
                d.grid_x = s->gx, d.grid_y = s->gy;
                out_tiles = (unsigned) (s->gx * s->gy);
                out_pitch = (size_t) vc_get_linesize(tw, c);
                lb = (size_t) (tw * get_bpp(c));
                rows = (size_t) h / (size_t) s->gy;
                break;
        }
        default: break;
        }
        if (out->tile_count < out_tiles) {
                MSG(ERROR, "the output frame has %u tiles, %u are needed\n", out->tile_count, out_tiles);
                return false;
        }
        const size_t tile_len = out_pitch * rows, out_len = tile_len * out_tiles;
        const struct tile *src[2] = { NULL, NULL };
        for (int i = 0; i < inputs; i++) { // (every tile is looked at before the first copy is queued: no return below skips the synchronisation)
                src[i] = s->kind == K_INTERLACE ? &s->in[i]->tiles[0] : &in->tiles[i];
                if (src[i]->data_len < in_len) {
                        MSG(ERROR, "frame shorter than %d lines of %zu bytes\n", h, L);
                        return false;
                }
        }
        if (!mi355x_gpu_enter(&s->gpu) || !reserve(s, in_len * (size_t) inputs, in_len, inputs, out_len)) {
                return false;
        }
        bool ok = true;
        for (int i = 0; ok && i < inputs; i++) {
                char *const pinned = (char *) s->host.ptr + (size_t) i * in_len;
                memcpy(pinned, src[i]->data, in_len);
                ok = ug_hip_upload_ordered_ex(s->gpu.device, s->dev_in[i].ptr, pinned, in_len, UG_HIP_MEMCPY_HOST_TO_DEVICE, s->gpu.stream, 0) == UG_HIP_SUCCESS;
        }
        d.src = s->dev_in[0].ptr, d.src2 = inputs == 2 ? s->dev_in[1].ptr : NULL, d.dst = s->dev_out.ptr;
        ok = ok && ug_hip_compose(&d, s->gpu.stream) == UG_HIP_SUCCESS;
        const size_t pitch = s->kind == K_SPLIT ? out_pitch : (size_t) req_pitch; // (vf_split writes its tiles packed, whatever req_pitch says)
        for (unsigned t = 0; ok && t < out_tiles; t++) {
                if (s->kind == K_SPLIT) { // vf_split.cpp:69-76
                        out->tiles[t].width = s->in_desc.width / (unsigned) s->gx;
                        out->tiles[t].height = (unsigned) rows;
                        out->tiles[t].data_len = (unsigned) tile_len;
                }
                ok = pitch >= lb && ug_hip_download_2d_ordered_ex(s->gpu.device, out->tiles[t].data, pitch, (char *) s->dev_out.ptr + t * tile_len, out_pitch, lb, rows, s->gpu.stream, 0) ==
                                            UG_HIP_SUCCESS;
        }
        if (s->kind == K_SPLIT) {
                out->color_spec = in->color_spec;
                out->fps = in->fps;
        }
        return mi355x_gpu_finish(&s->gpu, ok, kind_names[s->kind]);
}

// ---- crop as a capture filter (crop.c:200-234) ----
static struct video_frame *crop_filter(void *state, struct video_frame *f)
{
        struct state_cmp_mi355x *s = state;
        if (f == nullptr) {
                return nullptr;
        }
        if (s->in[0] == NULL || !video_desc_eq(s->in_desc, video_desc_from_frame(f))) {
                if (!reconfigure(s, video_desc_from_frame(f))) {
                        VIDEO_FRAME_DISPOSE(f);
                        return NULL;
                }
        }
        if (s->out_desc.width < 1) {
                VIDEO_FRAME_DISPOSE(f);
                return NULL;
        }
        struct video_frame *out = vf_alloc_desc_data(s->out_desc);
        out->callbacks.dispose = vf_free;
        const bool ok = postprocess(s, f, out, vc_get_linesize(s->out_desc.width, f->color_spec));
        VIDEO_FRAME_DISPOSE(f);
        if (!ok) {
                vf_free(out);
                return NULL;
        }
        return out;
}

// ---- logo (logo.c:162-235): in place, only the lines of the rectangle travel ----
static struct video_frame *logo_filter(void *state, struct video_frame *in)
{
        struct state_cmp_mi355x *s = state;
        if (in == nullptr) {
                return nullptr;
        }
        const codec_t c = in->color_spec;
        const ug_pixfmt_t fmt = ug_pixfmt_from_codec(c);
        if (ug_hip_compose_supported(UG_CMP_LOGO, fmt) != 1) {
                MSG(ERROR, "Cannot find decoder from %s to RGB and back!\n", get_codec_name(c));
                return in;
        }
        const int w = (int) in->tiles[0].width, h = (int) in->tiles[0].height;
        int rx = 0, ry = 0;
        if (ug_hip_logo_geometry(fmt, w, h, (int) s->lw, (int) s->lh, s->x, s->y, &rx, &ry) != UG_HIP_SUCCESS || rx < 0 || ry < 0) {
                return in;
        }
        if (rx + (int) s->lw > w || ry + (int) s->lh > h) { // the reference's rounding lets this through and draws across the line ends
                MSG(ERROR, "the logo (%ux%u) does not fit the frame (%dx%d)\n", s->lw, s->lh, w, h);
                return in;
        }
        const size_t L = (size_t) vc_get_linesize((unsigned) w, c), len = L * s->lh;
        char *const lines = in->tiles[0].data + (size_t) ry * L;
        if (!mi355x_gpu_enter(&s->gpu) || !reserve(s, len, len, 1, 0)) {
                return in;
        }
        struct ug_compose_desc d = { .dst = s->dev_in[0].ptr, .op = UG_CMP_LOGO, .format = fmt, .width = w, .lines = (int) s->lh, .frames = 1, .logo = s->logo_dev.ptr,
                                     .logo_w = (int) s->lw, .logo_h = (int) s->lh, .rect_x = rx, .rect_y = 0 };
        memcpy(s->host.ptr, lines, len);
        const bool ok = ug_hip_upload_ordered_ex(s->gpu.device, s->dev_in[0].ptr, s->host.ptr, len, UG_HIP_MEMCPY_HOST_TO_DEVICE, s->gpu.stream, 0) == UG_HIP_SUCCESS &&
                        ug_hip_compose(&d, s->gpu.stream) == UG_HIP_SUCCESS &&
                        ug_hip_download_2d_ordered_ex(s->gpu.device, lines, L, s->dev_in[0].ptr, L, L, s->lh, s->gpu.stream, 0) == UG_HIP_SUCCESS;
        mi355x_gpu_finish(&s->gpu, ok, kind_names[s->kind]);
        return in;
}

#define CMP_PP(name, kind, prop)                                                                                                                       \
        static void *init_##name(const char *cfg) { return init_common(kind, cfg); }                                                                    \
        static const struct vo_postprocess_info vo_pp_##name = { init_##name, reconfigure, getf, get_out_desc, prop, postprocess, done };               \
        REGISTER_MODULE(name, &vo_pp_##name, LIBRARY_CLASS_VIDEO_POSTPROCESS, VO_PP_ABI_VERSION);
#define CMP_CF(name, kind, fn)                                                                                                                          \
        static int cf_init_##name(struct module *parent, const char *cfg, void **state)                                                                 \
        {                                                                                                                                               \
                (void) parent;                                                                                                                          \
                if (strcmp(cfg, "help") == 0 || (kind == K_LOGO && strlen(cfg) == 0)) {                                                                 \
                        init_common(kind, "help");                                                                                                      \
                        return 1;                                                                                                                       \
                }                                                                                                                                       \
                *state = init_common(kind, cfg);                                                                                                        \
                return *state != NULL ? 0 : -1;                                                                                                         \
        }                                                                                                                                               \
        static const struct capture_filter_info capture_filter_##name = { .init = cf_init_##name, .done = done, .filter = fn };                         \
        REGISTER_MODULE(name, &capture_filter_##name, LIBRARY_CLASS_CAPTURE_FILTER, CAPTURE_FILTER_ABI_VERSION);

CMP_PP(crop_mi355x, K_CROP, get_property)
CMP_CF(crop_mi355x, K_CROP, crop_filter)
CMP_PP(border_mi355x, K_BORDER, get_property)
CMP_PP(interlace_mi355x, K_INTERLACE, get_property)
ADD_CAPTURE_FILTER_VO_PP_WRAPPER(interlace_mi355x, init_interlace_mi355x, reconfigure, get_out_desc, postprocess, done)
CMP_PP(interlaced_3d_mi355x, K_3D, get_property)
CMP_PP(split_mi355x, K_SPLIT, split_get_property)
CMP_CF(logo_mi355x, K_LOGO, logo_filter)
