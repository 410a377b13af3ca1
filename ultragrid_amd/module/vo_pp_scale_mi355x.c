/**
 * @file vo_pp_scale_mi355x.c
 * UltraGrid video postprocessor "scale_mi355x": `-p scale_mi355x:<width>:<height>` -- the reference's `scale` postprocessor
 * (src/vo_postprocess/scale.c) on an MI355X through libug_mi355x.so (include/ug_mi355x.h: ug_hip_scale), with no GL context.  Where the
 * build has no GL `scale` module (configure decided scale=no: MI355X_NO_SCALE_PP, integration/ultragrid_mi355x.patch) it also registers as
 * `scale`, as a drop-in.
 *
 * Same interface as scale.c: options `<w>:<h>`, both > 0 (else usage and NULL; `help` prints usage); codecs UYVY and RGBA
 * (VO_PP_PROPERTY_CODECS); getf hands out the module's own input frame -- here in pinned host memory; postprocess(NULL) returns false;
 * get_out_desc: the scaled size, the input's codec, interlacing and fps, one tile, DISPLAY_PROPERTY_VIDEO_MERGED.
 * postprocess: upload, ug_hip_scale into a packed device picture, ONE 2-D download at req_pitch (ug_hip_download_2d_ordered_ex), then the
 * state's stream is synchronised -- also on failure: nothing asynchronous is left pending when it returns.
 * Refused at reconfigure (the reference computes garbage there): tile_count != 1 (scale.c writes out->tiles[i] of a one-tile
 * frame), INTERLACED_MERGED with an odd output height (scale.c leaves the last line unwritten).  Odd UYVY widths take (w + 1) / 2 pairs per
 * line (the reference's rows shear).  The GPU: --param mi355x-device / -D (mi355x_receiver.h).
 */
#include <stdbool.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#ifdef HAVE_CONFIG_H
#include "config.h" // MI355X_NO_SCALE_PP (integration/ultragrid_mi355x.patch)
#endif
#include "debug.h"
#include "lib_common.h"
#include "types.h"
#include "video_codec.h"
#include "video_display.h"
#include "video_frame.h"
#include "vo_postprocess.h"

#include "mi355x_gpu_state.h"

#define MOD_NAME "[scale MI355X] "

struct state_scale_mi355x {
        int                 scaled_width, scaled_height;
        struct mi355x_gpu   gpu;
        struct video_desc   desc;
        struct video_frame *in; ///< getf's frame; its data = host_in
        struct mi355x_buf   host_in, dev_in, dev_out; ///< host_in: pinned
        size_t              in_len, out_linesize;
};

static unsigned scale_mi355x_state_count; // the states of this process take the listed devices in turn

static void usage(void)
{
        printf("Scale postprocessor settings (MI355X):\n");
        printf("\t-p scale_mi355x:width:height\n");
}

static bool scale_mi355x_get_property(void *state, int property, void *val, size_t *len)
{
        (void) state;
        const codec_t supported[] = { UYVY, RGBA }; // scale.c:68
        if (property != VO_PP_PROPERTY_CODECS) {
                return false;
        }
        if (*len < sizeof supported) {
                MSG(ERROR, "query little space.\n");
                *len = 0;
        } else {
                memcpy(val, supported, sizeof supported);
                *len = sizeof supported;
        }
        return true;
}

static void release(struct state_scale_mi355x *s)
{
        if (s->in) {
                s->in->tiles[0].data = NULL;
                vf_free(s->in);
                s->in = NULL;
        }
        mi355x_buf_release(&s->host_in);
        mi355x_buf_release(&s->dev_in);
        mi355x_buf_release(&s->dev_out);
}

static void *scale_mi355x_init(const char *config)
{
        if (strcmp(config, "help") == 0) {
                usage();
                return NULL;
        }
        int w = 0, h = 0;
        char *tmp = strdup(config), *save_ptr = NULL, *ptr;
        if ((ptr = strtok_r(tmp, ":", &save_ptr)) != NULL) w = atoi(ptr);
        if ((ptr = strtok_r(NULL, ":", &save_ptr)) != NULL) h = atoi(ptr);
        free(tmp);
        if (w <= 0 || h <= 0 || w > 65536 || h > 65536) {
                MSG(ERROR, "incorrect usage.\n");
                usage();
                return NULL;
        }
        struct state_scale_mi355x *s = calloc(1, sizeof *s);
        if (s == NULL) {
                return NULL;
        }
        s->scaled_width = w;
        s->scaled_height = h;
        s->host_in.pinned = true;
        if (!mi355x_gpu_open(&s->gpu, &scale_mi355x_state_count, MOD_NAME)) {
                free(s);
                return NULL;
        }
        return s;
}

static bool scale_mi355x_reconfigure(void *state, struct video_desc desc)
{
        struct state_scale_mi355x *s = state;
        if (!mi355x_gpu_enter(&s->gpu)) {
                return false;
        }
        release(s);
        if (desc.color_spec != UYVY && desc.color_spec != RGBA) {
                MSG(ERROR, "codec %s is not UYVY or RGBA\n", get_codec_name(desc.color_spec));
                return false;
        }
        if (desc.tile_count != 1) {
                MSG(ERROR, "%u tiles: only a one-tile frame is scaled (the output has one tile)\n", desc.tile_count);
                return false;
        }
        const bool merged = desc.interlacing == INTERLACED_MERGED;
        if (merged && (s->scaled_height % 2 != 0 || desc.height < 2)) {
                MSG(ERROR, "an interlaced (merged) picture needs an even output height and two lines in\n");
                return false;
        }
        if (desc.width == 0 || desc.height == 0 || desc.width > 65536 || desc.height > 65536) {
                MSG(ERROR, "frame size %ux%u out of range\n", desc.width, desc.height);
                return false;
        }
        s->desc = desc;
        s->in_len = (size_t) vc_get_linesize(desc.width, desc.color_spec) * desc.height;
        s->out_linesize = (size_t) vc_get_linesize((unsigned) s->scaled_width, desc.color_spec);
        s->in = vf_alloc_desc(desc);
        if (s->in == NULL || !mi355x_buf_reserve(&s->host_in, s->in_len) || !mi355x_buf_reserve(&s->dev_in, s->in_len) ||
            !mi355x_buf_reserve(&s->dev_out, s->out_linesize * (size_t) s->scaled_height)) {
                MSG(ERROR, "cannot allocate the frame buffers: %s\n", ug_hip_last_error_string());
                release(s);
                return false;
        }
        s->in->tiles[0].data = s->host_in.ptr;
        s->in->tiles[0].data_len = (unsigned) s->in_len;
        return true;
}

static struct video_frame *scale_mi355x_getf(void *state)
{
        return ((struct state_scale_mi355x *) state)->in;
}

static bool scale_mi355x_postprocess(void *state, struct video_frame *in, struct video_frame *out, int req_pitch)
{
        struct state_scale_mi355x *s = state;
        if (in == NULL) {
                return false;
        }
        if (s->in == NULL || in->tile_count != 1 || out == NULL || out->tiles[0].data == NULL) {
                MSG(ERROR, "not configured\n");
                return false;
        }
        if (req_pitch < 0 || (size_t) req_pitch < s->out_linesize) {
                MSG(ERROR, "pitch %d is shorter than a line of %zu bytes\n", req_pitch, s->out_linesize);
                return false;
        }
        if (!mi355x_gpu_enter(&s->gpu)) {
                return false;
        }
        const struct ug_scale_desc d = {
                .src = s->dev_in.ptr, .dst = s->dev_out.ptr, .format = s->desc.color_spec == UYVY ? UG_PF_UYVY : UG_PF_RGBA,
                .interlaced_merged = s->desc.interlacing == INTERLACED_MERGED,
                .src_width = (int) s->desc.width, .src_height = (int) s->desc.height,
                .dst_width = s->scaled_width, .dst_height = s->scaled_height, .frames = 1,
        };
        const bool ok = ug_hip_upload_ordered_ex(s->gpu.device, s->dev_in.ptr, in->tiles[0].data, s->in_len, UG_HIP_MEMCPY_HOST_TO_DEVICE, s->gpu.stream, 0) == UG_HIP_SUCCESS &&
                        ug_hip_scale(&d, s->gpu.stream) == UG_HIP_SUCCESS &&
                        ug_hip_download_2d_ordered_ex(s->gpu.device, out->tiles[0].data, (size_t) req_pitch, s->dev_out.ptr, s->out_linesize, s->out_linesize,
                                                      (size_t) s->scaled_height, s->gpu.stream, 0) == UG_HIP_SUCCESS;
        if (!ok) MSG(ERROR, "scale failed: %s\n", ug_hip_last_error_string()); // (said here: the bare word as a string of this object is what registering as `scale` leaves)
        return mi355x_gpu_finish(&s->gpu, ok, NULL); // (the caller reuses both frames)
}

static void scale_mi355x_get_out_desc(void *state, struct video_desc *out, int *in_display_mode)
{
        struct state_scale_mi355x *s = state;
        out->width = (unsigned) s->scaled_width;
        out->height = (unsigned) s->scaled_height;
        out->color_spec = s->desc.color_spec;
        out->interlacing = s->desc.interlacing;
        out->fps = s->desc.fps;
        out->tile_count = 1;
        *in_display_mode = DISPLAY_PROPERTY_VIDEO_MERGED;
}

static void scale_mi355x_done(void *state)
{
        struct state_scale_mi355x *s = state;
        mi355x_gpu_close(&s->gpu); // (the device stays the current one: the buffers go after the stream has been waited for)
        release(s);
        free(s);
}

static const struct vo_postprocess_info vo_pp_scale_mi355x_info = {
        scale_mi355x_init,
        scale_mi355x_reconfigure,
        scale_mi355x_getf,
        scale_mi355x_get_out_desc,
        scale_mi355x_get_property,
        scale_mi355x_postprocess,
        scale_mi355x_done,
};

REGISTER_MODULE(scale_mi355x, &vo_pp_scale_mi355x_info, LIBRARY_CLASS_VIDEO_POSTPROCESS, VO_PP_ABI_VERSION);
#ifdef MI355X_NO_SCALE_PP
REGISTER_MODULE(scale, &vo_pp_scale_mi355x_info, LIBRARY_CLASS_VIDEO_POSTPROCESS, VO_PP_ABI_VERSION);
#endif
