/**
 * @file ug_deint_harness.c
 * The de-interlacers through UltraGrid's own framework: src/vo_postprocess.c + the lib_common registry, with vo_pp_deinterlace_mi355x.o AND
 * the reference's own src/vo_postprocess/deinterlace.c and temporal-deint.c (compiled unmodified) linked in -- one process pushes the same
 * frames through `double_framerate` (the reference, CPU) and `double_framerate_mi355x` and writes both results.
 *
 * usage: ug_deint_harness list      the VIDEO_POSTPROCESS and CAPTURE_FILTER names of the registry
 *        ug_deint_harness run <name>[+<name>...] <options> <codec> <prog|merged> <extra pitch bytes> <out prefix> <reps> <w> <h> <in.raw> [<w> <h> <in.raw> ...]
 *            per name: vo_postprocess_init("<name>[:<options>]") (options "-" = none); per frame: vo_postprocess_reconfigure when the size changes
 *            (first frame included) -> get_out_desc -> getf -> the input bytes into it -> vo_postprocess(in, out, req_pitch = vc_get_linesize(w) +
 *            extra) into a frame pre-filled with 0xA5 -> <prefix>.<name>.<i>.0; vo_postprocess(NULL, out) into a pre-filled frame ->
 *            <prefix>.<name>.<i>.1 when it returned true; vo_postprocess(NULL) once more.  The whole sequence <reps> times (files of the last).
 *            stdout per frame: "<name> frame <i> <w> <h> <codec> <interlacing> <fps> <tile_count> <display mode> ret=<a><b><c>", and per name
 *            "<name> ms_per_frame=<wall-clock ms per input frame, all calls>"
 *            The output frames are allocated six lines longer than written to the files: the reference's avg_lines walks past the frame for R10k.
 * UG_PARAM=<k>=<v>[,...] answers get_commandline_param (e.g. mi355x-device=0).  Exit 0 = all frames processed, 2 = init refused, 3 = reconfigure
 * refused, 4 = postprocess failed.
 */
#include <stdbool.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "capture_filter.h"
#include "debug.h"
#include "lib_common.h"
#include "types.h"
#include "video_codec.h"
#include "video_display.h"
#include "video_frame.h"
#include "vo_postprocess.h"

#define UG_HARNESS_NAME "ug_deint_harness"
#include "ug_harness_host.h" /* what host.cpp would provide; get_commandline_param answers from UG_PARAM */

static bool write_file(const char *prefix, const char *name, int i, int k, const char *data, size_t len)
{
        char path[1024];
        snprintf(path, sizeof path, "%s.%s.%d.%d", prefix, name, i, k);
        FILE *f = fopen(path, "wb");
        const bool ok = f != NULL && fwrite(data, 1, len, f) == len;
        if (f) fclose(f);
        if (!ok) perror(path);
        return ok;
}

static int run_one(const char *name, int argc, char **argv)
{
        char cfg[256];
        snprintf(cfg, sizeof cfg, "%s%s%s", name, strcmp(argv[3], "-") == 0 ? "" : ":", strcmp(argv[3], "-") == 0 ? "" : argv[3]);
        const codec_t codec = get_codec_from_name(argv[4]);
        const enum interlacing_t inter = strcmp(argv[5], "merged") == 0 ? INTERLACED_MERGED : PROGRESSIVE;
        const int extra = atoi(argv[6]), reps = atoi(argv[8]);
        const char *prefix = argv[7];
        struct vo_postprocess_state *s = vo_postprocess_init(cfg);
        if (s == NULL || codec == VIDEO_CODEC_NONE) {
                return 2;
        }
        struct video_desc cur = { 0 };
        struct video_frame *out = NULL;
        int rc = 0, frames = 0;
        struct timespec t0, t1;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        for (int rep = 0; rep < reps && rc == 0; rep++) {
                for (int a = 9, i = 0; a + 2 < argc && rc == 0; a += 3, i++, frames++) {
                        const struct video_desc desc = { .width = (unsigned) atoi(argv[a]), .height = (unsigned) atoi(argv[a + 1]), .color_spec = codec,
                                                         .interlacing = inter, .fps = 25.0, .tile_count = 1 };
                        if (desc.width != cur.width || desc.height != cur.height) {
                                if (!vo_postprocess_reconfigure(s, desc)) {
                                        rc = 3;
                                        break;
                                }
                                cur = desc;
                        }
                        struct video_desc od;
                        int mode = -1;
                        vo_postprocess_get_out_desc(s, &od, &mode);
                        if (out) {
                                free(out->tiles[0].data);
                                vf_free(out);
                        }
                        out = vf_alloc_desc(od);
                        const int pitch = vc_get_linesize(od.width, od.color_spec) + extra;
                        const size_t out_len = (size_t) pitch * od.height, alloc_len = out_len + 6 * (size_t) pitch;
                        out->tiles[0].data = malloc(alloc_len);
                        out->tiles[0].data_len = (unsigned) out_len;
                        struct video_frame *in = vo_postprocess_getf(s);
                        FILE *f = fopen(argv[a + 2], "rb");
                        const size_t n = f ? fread(in->tiles[0].data, 1, in->tiles[0].data_len, f) : 0;
                        if (f) fclose(f);
                        if (n != in->tiles[0].data_len) {
                                fprintf(stderr, "%s: %zu of %u bytes\n", argv[a + 2], n, in->tiles[0].data_len);
                                rc = 1;
                                break;
                        }
                        bool ret[3];
                        for (int k = 0; k < 3; k++) {
                                memset(out->tiles[0].data, 0xA5, alloc_len);
                                ret[k] = vo_postprocess(s, k == 0 ? in : NULL, out, pitch);
                                if (ret[k] && rep == reps - 1 && !write_file(prefix, name, i, k, out->tiles[0].data, out_len)) rc = 1;
                        }
                        if (rep == reps - 1) {
                                printf("%s frame %d %u %u %s %d %.3f %u %d ret=%d%d%d\n", name, i, od.width, od.height, get_codec_name(od.color_spec), (int) od.interlacing,
                                       od.fps, od.tile_count, mode, (int) ret[0], (int) ret[1], (int) ret[2]);
                        }
                        if (!ret[0]) rc = 4;
                }
        }
        clock_gettime(CLOCK_MONOTONIC, &t1);
        if (rc == 0 && frames > 0) {
                printf("%s ms_per_frame=%.4f\n", name, ((double) (t1.tv_sec - t0.tv_sec) * 1e3 + (double) (t1.tv_nsec - t0.tv_nsec) / 1e6) / frames);
        }
        if (out) {
                free(out->tiles[0].data);
                vf_free(out);
        }
        vo_postprocess_done(s);
        return rc;
}

int main(int argc, char **argv)
{
        if (argc == 2 && strcmp(argv[1], "list") == 0) {
                list_modules(LIBRARY_CLASS_VIDEO_POSTPROCESS, VO_PP_ABI_VERSION, true);
                printf("capture filters:\n");
                list_modules(LIBRARY_CLASS_CAPTURE_FILTER, CAPTURE_FILTER_ABI_VERSION, true);
                return 0;
        }
        if (argc >= 12 && strcmp(argv[1], "run") == 0 && (argc - 9) % 3 == 0) {
                char *names = strdup(argv[2]), *save = NULL;
                int rc = 0;
                for (char *name = strtok_r(names, "+", &save); name != NULL && rc == 0; name = strtok_r(NULL, "+", &save)) {
                        rc = run_one(name, argc, argv);
                }
                free(names);
                return rc;
        }
        fprintf(stderr, "usage: %s list | run <name>[+<name>...] <options|-> <codec> <prog|merged> <extra pitch> <out prefix> <reps> <w> <h> <in.raw> [...]\n", argv[0]);
        return 1;
}
