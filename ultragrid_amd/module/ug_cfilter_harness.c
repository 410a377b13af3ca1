/**
 * @file ug_cfilter_harness.c
 * The colour / mirror filters through UltraGrid's own frameworks: src/capture_filter.c and src/vo_postprocess.c + the lib_common registry, with
 * capture_filter_pixel_mi355x.o AND the reference's own src/capture_filter/{matrix,matrix2,grayscale,mirror,flip}.c and gamma.cpp (compiled
 * unmodified) linked in -- one process pushes the same frames through `matrix2` (the reference, CPU) and `matrix2_mi355x` and writes both results.
 *
 * usage: ug_cfilter_harness list      the VIDEO_POSTPROCESS and CAPTURE_FILTER names of the registry
 *        ug_cfilter_harness run <name>[+<name>...] <options> <codec> <cf|pp> <out prefix> <reps> <w> <h> <in.raw> [<w> <h> <in.raw> ...]
 *            cf: capture_filter_init("<name>[:<options>]") (options "-" = none); per frame a new frame holding the input bytes ->
 *                capture_filter() -> <prefix>.<name>.<i> when it returned a frame of its own
 *            pp: vo_postprocess_init; per frame: vo_postprocess_reconfigure when the size changes (first frame included) -> get_out_desc ->
 *                getf -> the input bytes into it -> vo_postprocess(in, out, req_pitch = vc_get_linesize) into a frame pre-filled with 0xA5 ->
 *                <prefix>.<name>.<i> when it returned true
 *            The whole sequence <reps> times (files of the last).  stdout: first "cpus=<get_nprocs()>" -- what std::thread::hardware_concurrency()
 *            answers, the number of slices of the reference's gamma --, then per frame
 *            "<name> frame <i> <w> <h> <codec> <interlacing> <fps> <tile_count> <data_len> ret=<new|same|null|true|false>", and per name
 *            "<name> ms_per_frame=<wall-clock ms per input frame inside capture_filter() / vo_postprocess(), file I/O left out>"
 * UG_CFILTER_PAD=1: every malloc of the process returns three times the bytes asked for plus 4 KiB, pre-filled with 0xA5.  What the comparison with
 *            the reference needs: its gamma leaves the tail of a frame it malloc'ed unwritten, and its matrix2 hands vc_copylineY416toV210 the
 *            length of the Y416 frame (matrix2.c:239-241), three times the v210 frame it writes to and reads from.
 * UG_PARAM=<k>=<v>[,...] answers get_commandline_param (e.g. mi355x-device=0).  Exit 0 = all frames processed, 2 = init refused, 3 = reconfigure
 * refused, 4 = a filter returned NULL / false.
 */
#include <stdbool.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/sysinfo.h>
#include <time.h>

#include "capture_filter.h"
#include "debug.h"
#include "lib_common.h"
#include "types.h"
#include "video_codec.h"
#include "video_display.h"
#include "video_frame.h"
#include "vo_postprocess.h"

#define UG_HARNESS_NAME "ug_cfilter_harness"
#include "ug_harness_host.h" /* what host.cpp would provide; get_commandline_param answers from UG_PARAM */

/* -Wl,--wrap=malloc (see UG_CFILTER_PAD above) */
void *__real_malloc(size_t size);
static int pad_mallocs;
void *__wrap_malloc(size_t size)
{
        if (!pad_mallocs || size > ((size_t) 1 << 30)) {
                return __real_malloc(size);
        }
        const size_t padded = 3 * size + 4096;
        void *p = __real_malloc(padded);
        if (p != NULL) memset(p, 0xA5, padded);
        return p;
}

static bool write_file(const char *prefix, const char *name, int i, const char *data, size_t len)
{
        char path[1024];
        snprintf(path, sizeof path, "%s.%s.%d", prefix, name, i);
        FILE *f = fopen(path, "wb");
        const bool ok = f != NULL && fwrite(data, 1, len, f) == len;
        if (f) fclose(f);
        if (!ok) perror(path);
        return ok;
}

static bool read_file(const char *path, char *data, size_t len)
{
        FILE *f = fopen(path, "rb");
        const size_t n = f ? fread(data, 1, len, f) : 0;
        if (f) fclose(f);
        if (n != len) fprintf(stderr, "%s: %zu of %zu bytes\n", path, n, len);
        return n == len;
}

static void report(const char *name, int i, struct video_desc d, unsigned data_len, const char *ret)
{
        printf("%s frame %d %u %u %s %d %.3f %u %u ret=%s\n", name, i, d.width, d.height, get_codec_name(d.color_spec), (int) d.interlacing, d.fps, d.tile_count,
               data_len, ret);
}

static int run_one(const char *name, int argc, char **argv)
{
        char cfg[512];
        snprintf(cfg, sizeof cfg, "%s%s%s", name, strcmp(argv[3], "-") == 0 ? "" : ":", strcmp(argv[3], "-") == 0 ? "" : argv[3]);
        const codec_t codec = get_codec_from_name(argv[4]);
        const bool pp = strcmp(argv[5], "pp") == 0;
        const char *prefix = argv[6];
        const int reps = atoi(argv[7]);
        struct vo_postprocess_state *ps = NULL;
        struct capture_filter *cs = NULL;
        if (codec == VIDEO_CODEC_NONE || (pp ? (ps = vo_postprocess_init(cfg)) == NULL : capture_filter_init(NULL, cfg, &cs) != 0)) {
                return 2;
        }
        struct video_desc cur = { 0 };
        int rc = 0, frames = 0;
        double spent = 0;
        for (int rep = 0; rep < reps && rc == 0; rep++) {
                const bool last = rep == reps - 1;
                for (int a = 8, i = 0; a + 2 < argc && rc == 0; a += 3, i++, frames++) {
                        const struct video_desc desc = { .width = (unsigned) atoi(argv[a]), .height = (unsigned) atoi(argv[a + 1]), .color_spec = codec,
                                                         .interlacing = PROGRESSIVE, .fps = 25.0, .tile_count = 1 };
                        if (!pp) {
                                struct video_frame *in = vf_alloc_desc_data(desc);
                                in->callbacks.dispose = vf_free;
                                if (!read_file(argv[a + 2], in->tiles[0].data, in->tiles[0].data_len)) {
                                        vf_free(in);
                                        rc = 1;
                                        break;
                                }
                                const double t0 = now_ms();
                                struct video_frame *out = capture_filter(cs, in);
                                spent += now_ms() - t0;
                                if (out == NULL) {
                                        if (last) report(name, i, desc, 0, "null");
                                        rc = 4;
                                        break;
                                }
                                if (last) {
                                        report(name, i, video_desc_from_frame(out), out->tiles[0].data_len, out == in ? "same" : "new");
                                        if (!write_file(prefix, name, i, out->tiles[0].data, out->tiles[0].data_len)) rc = 1;
                                }
                                VIDEO_FRAME_DISPOSE(out);
                                continue;
                        }
                        if (desc.width != cur.width || desc.height != cur.height) {
                                if (!vo_postprocess_reconfigure(ps, desc)) {
                                        rc = 3;
                                        break;
                                }
                                cur = desc;
                        }
                        struct video_desc od;
                        int mode = -1;
                        vo_postprocess_get_out_desc(ps, &od, &mode);
                        struct video_frame *out = vf_alloc_desc(od);
                        const int pitch = vc_get_linesize(od.width, od.color_spec);
                        const size_t out_len = (size_t) pitch * od.height, alloc_len = 3 * out_len + 4096;
                        out->tiles[0].data = malloc(alloc_len);
                        out->tiles[0].data_len = (unsigned) out_len;
                        memset(out->tiles[0].data, 0xA5, alloc_len);
                        struct video_frame *in = vo_postprocess_getf(ps);
                        bool ret = false;
                        if (!read_file(argv[a + 2], in->tiles[0].data, in->tiles[0].data_len)) {
                                rc = 1;
                        } else {
                                const double t0 = now_ms();
                                ret = vo_postprocess(ps, in, out, pitch);
                                spent += now_ms() - t0;
                                if (last) {
                                        report(name, i, od, (unsigned) out_len, ret ? "true" : "false");
                                        if (ret && !write_file(prefix, name, i, out->tiles[0].data, out_len)) rc = 1;
                                }
                                if (!ret) rc = 4;
                        }
                        free(out->tiles[0].data);
                        vf_free(out);
                }
        }
        if (rc == 0 && frames > 0) {
                printf("%s ms_per_frame=%.4f\n", name, spent / frames);
        }
        if (ps) vo_postprocess_done(ps);
        if (cs) capture_filter_destroy(cs);
        return rc;
}

int main(int argc, char **argv)
{
        const char *pad = getenv("UG_CFILTER_PAD");
        pad_mallocs = pad != NULL && strcmp(pad, "1") == 0;
        if (argc == 2 && strcmp(argv[1], "list") == 0) {
                list_modules(LIBRARY_CLASS_VIDEO_POSTPROCESS, VO_PP_ABI_VERSION, true);
                printf("capture filters:\n");
                list_modules(LIBRARY_CLASS_CAPTURE_FILTER, CAPTURE_FILTER_ABI_VERSION, true);
                return 0;
        }
        if (argc >= 11 && strcmp(argv[1], "run") == 0 && (argc - 8) % 3 == 0 && (strcmp(argv[5], "cf") == 0 || strcmp(argv[5], "pp") == 0)) {
                printf("cpus=%d\n", get_nprocs());
                char *names = strdup(argv[2]), *save = NULL;
                int rc = 0;
                for (char *name = strtok_r(names, "+", &save); name != NULL && rc == 0; name = strtok_r(NULL, "+", &save)) {
                        rc = run_one(name, argc, argv);
                }
                free(names);
                fflush(stdout);
                return rc;
        }
        fprintf(stderr, "usage: %s list | run <name>[+<name>...] <options|-> <codec> <cf|pp> <out prefix> <reps> <w> <h> <in.raw> [...]\n", argv[0]);
        return 1;
}
