/**
 * @file vo_pp_deinterlace_mi355x.c
 * UltraGrid's de-interlacers on an MI355X through libug_mi355x.so (include/ug_mi355x.h: ug_hip_deinterlace), as video postprocessors and
 * capture filters beside the reference's CPU modules (which exist in every build: no name is taken over):
 *
 *   deinterlace_mi355x, deinterlace_blend_mi355x   src/vo_postprocess/deinterlace.c      (vc_deinterlace_ex; option `force`)
 *   double_framerate_mi355x[:d]                    src/vo_postprocess/temporal-deint.c   (options `d`, `nodelay`, `force`)
 *   deinterlace_bob_mi355x, deinterlace_linear_mi355x                                    (the same options)
 *
 * Same interface as the reference's modules (VO_PP_ABI_VERSION 8): `help` prints the usage; get_out_desc: the input's size and codec -- the
 * three temporal ones PROGRESSIVE, fps * 2, DISPLAY_PROPERTY_VIDEO_MERGED; input that is not INTERLACED_MERGED and no `force`: a plain
 * copy; the temporal ones return a second frame from postprocess(NULL) once, then false, and wait half a frame time before it unless
 * `nodelay` (temporal-deint.c:499-510).  A codec the kernels do not take (ug_hip_deinterlace_supported) goes the reference's way on the host:
 * a copy (deinterlace), the weave without the blend, bob, linear with the lines between doubled.
 * postprocess(in): getf's frame lies in pinned host memory; one upload, ONE launch that computes both outputs (double_framerate: from this
 * frame and the previous one, which stays on the device), 2-D download(s) at req_pitch, and the state's stream is synchronised before it
 * returns -- also on failure.  The second output is downloaded during that call (into pinned memory) and only handed over by postprocess(NULL).
 * Where the reference leaves the end of an averaged line unwritten (R12L; include/ug_mi355x.h) those bytes of `out` are left alone here too.
 * Deviations: double_framerate with an odd height is refused at reconfigure (the reference copies a line past its buffers);
 * the previous-frame buffer starts zeroed (the reference's is uninitialised); req_pitch is honoured by `:d` and by the plain copy (the
 * reference blends and copies at the line size).  The GPU: --param mi355x-device / -D (mi355x_receiver.h).
 */
#include <stdbool.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#ifdef HAVE_CONFIG_H
#include "config.h"
#endif
#include "capture_filter.h"
#include "capture_filter/vo_pp_wrapper.h"
#include "compat/c23.h"
#include "debug.h"
#include "lib_common.h"
#include "tv.h"
#include "types.h"
#include "video_codec.h"
#include "video_display.h"
#include "video_frame.h"
#include "vo_postprocess.h"

#include "mi355x_gpu_state.h"
#include "ug_codec_map.h"

#define MOD_NAME "[deinterlace MI355X] "

enum deint_algo { ALGO_BLEND, ALGO_DF, ALGO_BOB, ALGO_LINEAR };

struct state_deint_mi355x {
        enum deint_algo     algo;
        bool                deinterlace, nodelay, force;
        bool                other_frame_emitted;
        time_ns_t           frame_received;
        struct mi355x_gpu   gpu;
        struct video_desc   desc;
        bool                active; ///< INTERLACED_MERGED or `force`: otherwise a copy
        bool                on_gpu; ///< the kernels take the codec
        struct video_frame *in;     ///< getf's frame; its data = host_in[cur]
        struct mi355x_buf   host_in[2], stage[2]; ///< pinned: the input frames in turn (the reference's buffers[]); packed outputs
        struct mi355x_buf   dev_in[2], dev_out[2];
        int                 cur;
        size_t              linesize, len, avg_bytes;
        int                 lines;
};

static unsigned deint_mi355x_state_count; // the states of this process take the listed devices in turn

static void usage(enum deint_algo algo)
{
        static const char *const names[] = { "deinterlace[_blend]_mi355x", "double_framerate_mi355x", "deinterlace_bob_mi355x", "deinterlace_linear_mi355x" };
        printf("De-interlacer on the MI355X:\n\t-p %s%s\n", names[algo], algo == ALGO_BLEND ? "[:force]" : "[:d|:nodelay|:force]");
        printf("\tforce   - apply even if the input is not interlaced\n");
        if (algo != ALGO_BLEND) {
                printf("\td       - blend the output lines (double_framerate)\n");
                printf("\tnodelay - do not wait half a frame time before the second frame\n");
        }
}

static void *init_common(enum deint_algo algo, const char *config)
{
        if (strcmp(config, "help") == 0) {
                usage(algo);
                return NULL;
        }
        bool d = false, nodelay = false, force = false;
        if (strcmp(config, "force") == 0) {
                force = true;
        } else if (algo != ALGO_BLEND && strcmp(config, "d") == 0) {
                d = true;
        } else if (algo != ALGO_BLEND && strcmp(config, "nodelay") == 0) {
                nodelay = true;
        } else if (strlen(config) > 0) {
                MSG(ERROR, "Unknown option: %s\n", config);
                return NULL;
        }
        struct state_deint_mi355x *s = calloc(1, sizeof *s);
        if (s == NULL) {
                return NULL;
        }
        s->algo = algo;
        s->deinterlace = d;
        s->nodelay = nodelay;
        s->force = force;
        s->host_in[0].pinned = s->host_in[1].pinned = s->stage[0].pinned = s->stage[1].pinned = true;
        if (!mi355x_gpu_open(&s->gpu, &deint_mi355x_state_count, MOD_NAME)) {
                free(s);
                return NULL;
        }
        if (nodelay && get_commandline_param("decoder-drop-policy") == NULL) { // temporal-deint.c:134-137
                set_commandline_param("decoder-drop-policy", "20ms");
        }
        return s;
}

static void *blend_init(const char *config) { return init_common(ALGO_BLEND, config); }
static void *df_init(const char *config) { return init_common(ALGO_DF, config); }
static void *bob_init(const char *config) { return init_common(ALGO_BOB, config); }
static void *linear_init(const char *config) { return init_common(ALGO_LINEAR, config); }

static bool deint_get_property(void *state, int property, void *val, size_t *len)
{
        (void) state, (void) property, (void) val, (void) len;
        return false;
}

static void release(struct state_deint_mi355x *s)
{
        if (s->in) {
                s->in->tiles[0].data = NULL;
                vf_free(s->in);
                s->in = NULL;
        }
        for (int i = 0; i < 2; i++) {
                mi355x_buf_release(&s->host_in[i]);
                mi355x_buf_release(&s->stage[i]);
                mi355x_buf_release(&s->dev_in[i]);
                mi355x_buf_release(&s->dev_out[i]);
        }
}

/// the bytes of a line that an averaged line writes (include/ug_mi355x.h; for vc_get_linesize line sizes only R12L leaves a rest)
static size_t averaged_bytes(codec_t codec, bool linear, size_t linesize)
{
        if (codec == R12L) {
                const size_t n = linear ? linesize / 16 * 4 : linesize / 36 * 8;
                return 4 * (n - (n % 3 != 0));
        }
        if (codec == v210 || (codec == R10k && !linear) || (get_bits_per_component(codec) == 16 && !linear && linesize >= 16)) {
                return linesize / 16 * 16;
        }
        return linesize;
}

static bool deint_reconfigure(void *state, struct video_desc desc)
{
        struct state_deint_mi355x *s = state;
        if (!mi355x_gpu_enter(&s->gpu)) {
                return false;
        }
        release(s);
        if (desc.tile_count != 1 || desc.width == 0 || desc.height == 0 || desc.width > 65536 || desc.height > 65536) {
                MSG(ERROR, "one tile of 1..65536 x 1..65536 pixels expected\n");
                return false;
        }
        s->active = desc.interlacing == INTERLACED_MERGED || s->force;
        if (s->algo != ALGO_BLEND && s->active && (desc.height < 2 || (s->algo == ALGO_DF && desc.height % 2 != 0))) {
                MSG(ERROR, "%u lines: the temporal de-interlacers need two lines, double_framerate an even number\n", desc.height);
                return false;
        }
        if (s->algo != ALGO_BLEND && !s->active) {
                MSG(WARNING, "the input is %s, not interlaced merged: every frame will simply be sent twice (`force` de-interlaces it anyway)\n",
                    get_interlacing_description(desc.interlacing));
        }
        static const int modes[] = { UG_DEINT_BLEND, UG_DEINT_WEAVE, UG_DEINT_BOB, UG_DEINT_LINEAR };
        s->on_gpu = ug_hip_deinterlace_supported(ug_pixfmt_from_codec(desc.color_spec), modes[s->algo]) == 1;
        if (s->active && !s->on_gpu) {
                MSG(WARNING, "pixel format '%s' is not de-interlaced on the GPU: %s on the host\n", get_codec_name(desc.color_spec),
                    s->algo == ALGO_BLEND ? "copying" : "weave / bob");
        }
        s->desc = desc;
        s->linesize = (size_t) vc_get_linesize(desc.width, desc.color_spec);
        s->lines = (int) desc.height;
        s->len = s->linesize * desc.height;
        s->avg_bytes = averaged_bytes(desc.color_spec, s->algo == ALGO_LINEAR, s->linesize);
        s->cur = 0;
        const int n = s->algo == ALGO_BLEND ? 1 : 2;
        bool ok = (s->in = vf_alloc_desc(desc)) != NULL;
        for (int i = 0; ok && i < n; i++) {
                ok = mi355x_buf_reserve(&s->host_in[i], s->len);
                if (ok) memset(s->host_in[i].ptr, 0, s->len); // the frame "before the first": zero (the reference's is uninitialised)
                if (ok && s->active && s->on_gpu) {
                        ok = mi355x_buf_reserve(&s->stage[i], s->len) && mi355x_buf_reserve(&s->dev_in[i], s->len) && mi355x_buf_reserve(&s->dev_out[i], s->len) &&
                             ug_hip_memset_async(s->dev_in[i].ptr, 0, s->len, s->gpu.stream) == UG_HIP_SUCCESS;
                }
        }
        ok = ok && ug_hip_stream_sync(s->gpu.stream) == UG_HIP_SUCCESS;
        if (!ok) {
                MSG(ERROR, "cannot allocate the frame buffers: %s\n", ug_hip_last_error_string());
                release(s);
                return false;
        }
        s->in->tiles[0].data = s->host_in[0].ptr;
        s->in->tiles[0].data_len = (unsigned) s->len;
        return true;
}

static struct video_frame *deint_getf(void *state)
{
        struct state_deint_mi355x *s = state;
        if (s->in != NULL && s->algo != ALGO_BLEND) { // the input frames in turn: the one before stays where it is (temporal-deint.c:213-221)
                s->cur = (s->cur + 1) % 2;
                s->in->tiles[0].data = s->host_in[s->cur].ptr;
        }
        return s->in;
}

static void copy_lines(char *dst, size_t dpitch, const char *src, size_t spitch, size_t width, int first, int step, int end)
{
        for (int y = first; y < end; y += step) memcpy(dst + (size_t) y * dpitch, src + (size_t) y * spitch, width);
}

/// is line y of output `which` an averaged line of deinterlace_linear (perform_linear, temporal-deint.c:442-466)?
static bool linear_averaged(int lines, int which, int y)
{
        return which == 0 ? (y % 2 == 1 && y < 2 * ((lines - 1) / 2)) : (y % 2 == 0 && y >= 2 && y <= 2 * ((lines - 2) / 2));
}

/// a packed output picture -> out at req_pitch, the ends of averaged lines left alone where the reference does not write them
static void hand_over(const struct state_deint_mi355x *s, char *out, size_t pitch, const char *packed, int which)
{
        for (int y = 0; y < s->lines; y++) {
                const bool avg = s->algo == ALGO_LINEAR && linear_averaged(s->lines, which, y);
                memcpy(out + (size_t) y * pitch, packed + (size_t) y * s->linesize, avg ? s->avg_bytes : s->linesize);
        }
}

/// the reference's path for a codec its averages do not take, on the host: weave, bob, linear with the upper line doubled
static void host_temporal(const struct state_deint_mi355x *s, char *out, size_t pitch, int which)
{
        const char *cur = s->host_in[s->cur].ptr, *prev = s->host_in[1 - s->cur].ptr;
        const size_t L = s->linesize;
        const int H = s->lines;
        if (s->algo == ALGO_DF) {
                copy_lines(out, pitch, cur, L, L, 0, which == 0 ? 2 : 1, H);
                if (which == 0) copy_lines(out, pitch, prev, L, L, 1, 2, H);
                return;
        }
        for (int y = 0; y < H; y++) {
                int i;
                if (s->algo == ALGO_BOB) {
                        i = which == 0 ? (y & ~1) : (y == 0 ? 1 : ((y - 1) & ~1) + 1);
                        if (y == H - 1 && which == 0 && H % 2 == 1) i = H - 3;
                        if (y == H - 1 && which == 1 && H % 2 == 0) i = H == 2 ? 1 : H - 3;
                } else {
                        const int rest = which == 0 ? 2 * ((H - 1) / 2) : 2 * ((H - 2) / 2) + 1; // "last line(s)": all copies of the first of them
                        i = linear_averaged(H, which, y) ? y - 1 : (which == 1 && y == 0 ? 1 : (y > rest ? rest : y));
                }
                memcpy(out + (size_t) y * pitch, cur + (size_t) i * L, L);
        }
}

static bool run_gpu(struct state_deint_mi355x *s, char *out, size_t pitch)
{
        static const int modes[] = { UG_DEINT_BLEND, UG_DEINT_WEAVE, UG_DEINT_BOB, UG_DEINT_LINEAR };
        const struct ug_deinterlace_desc d = {
                .src = s->dev_in[s->cur].ptr, .prev = s->algo == ALGO_DF ? s->dev_in[1 - s->cur].ptr : NULL, .dst = { s->dev_out[0].ptr, s->dev_out[1].ptr },
                .format = ug_pixfmt_from_codec(s->desc.color_spec), .mode = modes[s->algo], .blend_after_weave = s->deinterlace && s->algo == ALGO_DF,
                .lines = s->lines, .linesize = s->linesize, .frames = 1,
        };
        const size_t L = s->linesize, rows = (size_t) s->lines;
        // BLEND: the averaged part of every line straight into `out`; LINEAR with unwritten line ends: through the packed pinned copy
        const bool staged = s->algo == ALGO_LINEAR && s->avg_bytes < L;
        const size_t width = s->algo == ALGO_BLEND && s->lines > 1 ? s->avg_bytes : L;
        bool ok = ug_hip_upload_ordered_ex(s->gpu.device, s->dev_in[s->cur].ptr, s->host_in[s->cur].ptr, s->len, UG_HIP_MEMCPY_HOST_TO_DEVICE, s->gpu.stream, 0) == UG_HIP_SUCCESS &&
                  ug_hip_deinterlace(&d, s->gpu.stream) == UG_HIP_SUCCESS;
        if (ok && width > 0) {
                ok = staged ? ug_hip_download_ordered_ex(s->gpu.device, s->stage[0].ptr, s->dev_out[0].ptr, s->len, s->gpu.stream, 0) == UG_HIP_SUCCESS
                            : ug_hip_download_2d_ordered_ex(s->gpu.device, out, pitch, s->dev_out[0].ptr, L, width, rows, s->gpu.stream, 0) == UG_HIP_SUCCESS;
        }
        if (ok && s->algo != ALGO_BLEND) {
                ok = ug_hip_download_ordered_ex(s->gpu.device, s->stage[1].ptr, s->dev_out[1].ptr, s->len, s->gpu.stream, 0) == UG_HIP_SUCCESS;
        }
        if (!mi355x_gpu_finish(&s->gpu, ok, "de-interlacing")) { // (the caller reuses both frames)
                return false;
        }
        if (staged) hand_over(s, out, pitch, s->stage[0].ptr, 0);
        if (s->algo == ALGO_BLEND && s->lines > 1 && width < L) { // "the last line": the L bytes of out's line above (video_codec.c:851)
                memcpy(out + (rows - 1) * pitch + width, out + (rows - 2) * pitch + width, L - width);
        }
        return true;
}

/// @param in may be NULL (the temporal ones: the second frame)
static bool deint_postprocess(void *state, struct video_frame *in, struct video_frame *out, int req_pitch)
{
        struct state_deint_mi355x *s = state;
        if (in == NULL) {
                if (s->algo == ALGO_BLEND || s->other_frame_emitted) {
                        return false;
                }
                s->other_frame_emitted = true;
        } else {
                s->other_frame_emitted = false;
        }
        if (s->in == NULL || out == NULL || out->tiles[0].data == NULL || (in != NULL && in->tile_count != 1)) {
                MSG(ERROR, "not configured\n");
                return false;
        }
        if (req_pitch < 0 || (size_t) req_pitch < s->linesize) {
                MSG(ERROR, "pitch %d is shorter than a line of %zu bytes\n", req_pitch, s->linesize);
                return false;
        }
        if (in != NULL && in != s->in) { // a capture filter's frame: into the module's own (pinned) one
                struct video_frame *own = deint_getf(s);
                memcpy(own->tiles[0].data, in->tiles[0].data, in->tiles[0].data_len < s->len ? in->tiles[0].data_len : s->len);
        }
        const size_t pitch = (size_t) req_pitch;
        char *o = out->tiles[0].data;
        bool ok = true;
        if (!s->active || (s->algo == ALGO_BLEND && !s->on_gpu)) {
                copy_lines(o, pitch, s->host_in[s->cur].ptr, s->linesize, s->linesize, 0, 1, s->lines);
        } else if (!s->on_gpu) {
                host_temporal(s, o, pitch, in == NULL);
        } else if (in != NULL) {
                if (!mi355x_gpu_enter(&s->gpu)) {
                        return false;
                }
                ok = run_gpu(s, o, pitch);
        } else {
                hand_over(s, o, pitch, s->stage[1].ptr, 1);
        }
        if (s->algo != ALGO_BLEND && !s->nodelay) { // not both frames in bulk: wait half of the frame time (temporal-deint.c:499-510)
                if (in != NULL) {
                        s->frame_received = get_time_in_ns();
                } else {
                        time_ns_t t = 0;
                        do {
                                t = get_time_in_ns();
                        } while (out->fps > 0 && NS_TO_SEC_DBL(t - s->frame_received) <= 0.5 / out->fps);
                }
        }
        return ok;
}

static void deint_get_out_desc(void *state, struct video_desc *out, int *in_display_mode)
{
        struct state_deint_mi355x *s = state;
        *out = s->desc;
        if (s->algo == ALGO_BLEND) { // deinterlace.c:205-215: the description of its frame, the display mode untouched
                return;
        }
        out->interlacing = PROGRESSIVE;
        out->fps = s->desc.fps * 2.0;
        out->tile_count = 1;
        *in_display_mode = DISPLAY_PROPERTY_VIDEO_MERGED;
}

static void deint_done(void *state)
{
        struct state_deint_mi355x *s = state;
        mi355x_gpu_close(&s->gpu); // (the device stays the current one: the buffers go after the stream has been waited for)
        release(s);
        free(s);
}

/* `--capture-filter deinterlace_mi355x` (deinterlace.c:109-122,181-195): a new frame per input frame */
static int cf_blend_init(struct module *parent, const char *cfg, void **state)
{
        (void) parent;
        void *s = blend_init(cfg);
        if (s == NULL) {
                return 1;
        }
        *state = s;
        return 0;
}

static struct video_frame *cf_blend_filter(void *state, struct video_frame *f)
{
        struct state_deint_mi355x *s = state;
        const struct video_desc desc = video_desc_from_frame(f);
        struct video_frame *out = NULL;
        if ((s->in != NULL && video_desc_eq(desc, s->desc)) || deint_reconfigure(s, desc)) {
                out = vf_alloc_desc_data(desc);
                out->interlacing = PROGRESSIVE;
                out->callbacks.dispose = vf_free;
                if (!deint_postprocess(s, f, out, vc_get_linesize(desc.width, desc.color_spec))) {
                        vf_free(out);
                        out = NULL;
                }
        }
        VIDEO_FRAME_DISPOSE(f);
        return out;
}

#define DEINT_INFO(name, init) \
        static const struct vo_postprocess_info vo_pp_##name##_info = { init, deint_reconfigure, deint_getf, deint_get_out_desc, deint_get_property, deint_postprocess, deint_done }
DEINT_INFO(deinterlace_blend_mi355x, blend_init);
DEINT_INFO(double_framerate_mi355x, df_init);
DEINT_INFO(deinterlace_bob_mi355x, bob_init);
DEINT_INFO(deinterlace_linear_mi355x, linear_init);

static const struct capture_filter_info capture_filter_deinterlace_mi355x_info = { cf_blend_init, deint_done, cf_blend_filter };

REGISTER_MODULE(deinterlace_blend_mi355x, &vo_pp_deinterlace_blend_mi355x_info, LIBRARY_CLASS_VIDEO_POSTPROCESS, VO_PP_ABI_VERSION);
REGISTER_MODULE(deinterlace_mi355x, &vo_pp_deinterlace_blend_mi355x_info, LIBRARY_CLASS_VIDEO_POSTPROCESS, VO_PP_ABI_VERSION);
REGISTER_MODULE(deinterlace_mi355x, &capture_filter_deinterlace_mi355x_info, LIBRARY_CLASS_CAPTURE_FILTER, CAPTURE_FILTER_ABI_VERSION);
REGISTER_MODULE(double_framerate_mi355x, &vo_pp_double_framerate_mi355x_info, LIBRARY_CLASS_VIDEO_POSTPROCESS, VO_PP_ABI_VERSION);
ADD_CAPTURE_FILTER_VO_PP_WRAPPER(double_framerate_mi355x, df_init, deint_reconfigure, deint_get_out_desc, deint_postprocess, deint_done);
REGISTER_MODULE(deinterlace_bob_mi355x, &vo_pp_deinterlace_bob_mi355x_info, LIBRARY_CLASS_VIDEO_POSTPROCESS, VO_PP_ABI_VERSION);
ADD_CAPTURE_FILTER_VO_PP_WRAPPER(deinterlace_bob_mi355x, bob_init, deint_reconfigure, deint_get_out_desc, deint_postprocess, deint_done);
REGISTER_MODULE(deinterlace_linear_mi355x, &vo_pp_deinterlace_linear_mi355x_info, LIBRARY_CLASS_VIDEO_POSTPROCESS, VO_PP_ABI_VERSION);
ADD_CAPTURE_FILTER_VO_PP_WRAPPER(deinterlace_linear_mi355x, linear_init, deint_reconfigure, deint_get_out_desc, deint_postprocess, deint_done);
