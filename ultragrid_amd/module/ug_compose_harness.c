/**
 * @file ug_compose_harness.c
 * The geometric / compositing filters through UltraGrid's own frameworks: src/vo_postprocess.c and src/capture_filter.c + the lib_common registry,
 * with the reference's own src/vo_postprocess/{crop,border,interlace,3d-interlaced,split}.c, src/capture_filter/logo.c and src/utils/vf_split.cpp
 * (compiled unmodified, where they lie) linked in -- and whatever *_mi355x module the build adds beside them: one process pushes the same frames
 * through every name of a `+` list and writes each result.
 *
 * usage: ug_compose_harness list      the VIDEO_POSTPROCESS and CAPTURE_FILTER names of the registry
 *        ug_compose_harness run <name>[+<name>...] <options> <codec> <cf|pp> <tiles> <out prefix> <w> <h> <in.raw> [<w> <h> <in.raw> ...]
 *            <in.raw> holds <tiles> tiles of vc_get_linesize(w) * h bytes back to back (interlaced_3d: 2).  Options "-" = none.
 *            pp: vo_postprocess_init("<name>[:<options>]"); per frame: vo_postprocess_reconfigure when the size changes (first frame included) ->
 *                get_out_desc -> getf -> the input bytes into its tiles -> vo_postprocess(in, out, req_pitch = vc_get_linesize(out width)) into a
 *                frame of get_out_desc's tile count -> <prefix>.<name>.<i> (the tiles back to back) when it returned true
 *            cf: capture_filter_init; per frame a frame of the harness's own holding the input bytes -> capture_filter() -> <prefix>.<name>.<i>
 *                when it returned a frame
 *            Every buffer the harness hands out -- the pp output tiles, the cf input frame -- is allocated three times its size plus 4 KiB and
 *            pre-filled with 0xA5; `pad` counts the bytes behind the buffer's own length that no longer hold 0xA5 (a frame the filter allocated
 *            itself: pad=-1).  A filter that answers false / NULL (interlace on the first frame of a pair) is reported and the run goes on.
 *            stdout per frame: "<name> frame <i> <w> <h> <codec> <interlacing> <fps> <tile_count> <data_len> <display mode> ret=<true|false|new|same|null>
 *            pad=<n>", per name "<name> ms_per_frame=<wall-clock ms per input frame inside the filter>"
 * UG_PARAM=<k>=<v>[,...] answers get_commandline_param (e.g. mi355x-device=0).  Exit 0 = all frames pushed, 2 = init refused, 3 = reconfigure refused.
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

#define UG_HARNESS_NAME "ug_compose_harness"
#include "ug_harness_host.h" /* what host.cpp would provide; get_commandline_param answers from UG_PARAM */

enum { FILL = 0xA5 };
static size_t padded(size_t len) { return 3 * len + 4096; }
static char *alloc_padded(size_t len)
{
        char *p = malloc(padded(len));
        if (p != NULL) memset(p, FILL, padded(len));
        return p;
}
static long pad_changed(const char *p, size_t len)
{
        long n = 0;
        for (size_t i = len; i < padded(len); i++) n += (unsigned char) p[i] != FILL;
        return n;
}

static void report(const char *name, int i, struct video_desc d, unsigned data_len, int mode, const char *ret, long pad)
{
        printf("%s frame %d %u %u %s %d %.3f %u %u %d ret=%s pad=%ld\n", name, i, d.width, d.height, get_codec_name(d.color_spec), (int) d.interlacing, d.fps,
               d.tile_count, data_len, mode, ret, pad);
}

static FILE *open_out(const char *prefix, const char *name, int i)
{
        char path[1024];
        snprintf(path, sizeof path, "%s.%s.%d", prefix, name, i);
        FILE *f = fopen(path, "wb");
        if (f == NULL) perror(path);
        return f;
}

static void free_own_frame(struct video_frame *f)
{
        for (unsigned t = 0; t < f->tile_count; t++) free(f->tiles[t].data);
        vf_free(f);
}

static int run_one(const char *name, int argc, char **argv)
{
        char cfg[1024];
        snprintf(cfg, sizeof cfg, "%s%s%s", name, strcmp(argv[3], "-") == 0 ? "" : ":", strcmp(argv[3], "-") == 0 ? "" : argv[3]);
        const codec_t codec = get_codec_from_name(argv[4]);
        const bool pp = strcmp(argv[5], "pp") == 0;
        const unsigned tiles = (unsigned) atoi(argv[6]);
        const char *prefix = argv[7];
        struct vo_postprocess_state *ps = NULL;
        struct capture_filter *cs = NULL;
        if (codec == VIDEO_CODEC_NONE || tiles < 1 || tiles > 2 || (pp ? (ps = vo_postprocess_init(cfg)) == NULL : capture_filter_init(NULL, cfg, &cs) != 0)) {
                return 2;
        }
        struct video_desc cur = { 0 };
        int rc = 0, frames = 0;
        double spent = 0;
        for (int a = 8, i = 0; a + 2 < argc && rc == 0; a += 3, i++, frames++) {
                const struct video_desc desc = { .width = (unsigned) atoi(argv[a]), .height = (unsigned) atoi(argv[a + 1]), .color_spec = codec,
                                                 .interlacing = PROGRESSIVE, .fps = 25.0, .tile_count = tiles };
                const size_t in_len = (size_t) vc_get_linesize(desc.width, codec) * desc.height;
                FILE *fin = fopen(argv[a + 2], "rb");
                if (fin == NULL) {
                        perror(argv[a + 2]);
                        rc = 1;
                        break;
                }
                if (!pp) {
                        struct video_frame *in = vf_alloc_desc(desc);
                        in->callbacks.dispose = free_own_frame;
                        bool ok = true;
                        for (unsigned t = 0; t < tiles; t++) {
                                in->tiles[t].data = alloc_padded(in_len);
                                in->tiles[t].data_len = (unsigned) in_len;
                                ok = ok && fread(in->tiles[t].data, 1, in_len, fin) == in_len;
                        }
                        fclose(fin);
                        if (!ok) {
                                fprintf(stderr, "%s: short\n", argv[a + 2]);
                                free_own_frame(in);
                                rc = 1;
                                break;
                        }
                        const double t0 = now_ms();
                        struct video_frame *out = capture_filter(cs, in);
                        spent += now_ms() - t0;
                        if (out == NULL) {
                                report(name, i, desc, 0, -1, "null", -1);
                                continue;
                        }
                        report(name, i, video_desc_from_frame(out), out->tiles[0].data_len, -1, out == in ? "same" : "new",
                               out == in ? pad_changed(out->tiles[0].data, in_len) : -1);
                        FILE *fo = open_out(prefix, name, i);
                        if (fo == NULL || fwrite(out->tiles[0].data, 1, out->tiles[0].data_len, fo) != out->tiles[0].data_len) rc = 1;
                        if (fo) fclose(fo);
                        VIDEO_FRAME_DISPOSE(out);
                        continue;
                }
                if (desc.width != cur.width || desc.height != cur.height) {
                        if (!vo_postprocess_reconfigure(ps, desc)) {
                                fclose(fin);
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
                const size_t out_len = (size_t) pitch * od.height;
                for (unsigned t = 0; t < od.tile_count; t++) {
                        out->tiles[t].data = alloc_padded(out_len);
                        out->tiles[t].data_len = (unsigned) out_len;
                }
                struct video_frame *in = vo_postprocess_getf(ps);
                bool ok = in != NULL && in->tile_count >= tiles;
                for (unsigned t = 0; ok && t < tiles; t++) ok = in->tiles[t].data_len >= in_len && fread(in->tiles[t].data, 1, in_len, fin) == in_len;
                fclose(fin);
                if (!ok) {
                        fprintf(stderr, "%s: short, or the filter's frame does not hold it\n", argv[a + 2]);
                        rc = 1;
                } else {
                        const double t0 = now_ms();
                        const bool ret = vo_postprocess(ps, in, out, pitch);
                        spent += now_ms() - t0;
                        long pad = 0;
                        for (unsigned t = 0; t < od.tile_count; t++) pad += pad_changed(out->tiles[t].data, out_len);
                        report(name, i, od, (unsigned) out_len, mode, ret ? "true" : "false", pad);
                        if (ret) {
                                FILE *fo = open_out(prefix, name, i);
                                for (unsigned t = 0; fo != NULL && t < od.tile_count; t++) {
                                        if (fwrite(out->tiles[t].data, 1, out_len, fo) != out_len) rc = 1;
                                }
                                if (fo) fclose(fo);
                                else rc = 1;
                        }
                }
                free_own_frame(out);
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
        if (argc == 2 && strcmp(argv[1], "list") == 0) {
                list_modules(LIBRARY_CLASS_VIDEO_POSTPROCESS, VO_PP_ABI_VERSION, true);
                printf("capture filters:\n");
                list_modules(LIBRARY_CLASS_CAPTURE_FILTER, CAPTURE_FILTER_ABI_VERSION, true);
                return 0;
        }
        if (argc >= 11 && strcmp(argv[1], "run") == 0 && (argc - 8) % 3 == 0 && (strcmp(argv[5], "cf") == 0 || strcmp(argv[5], "pp") == 0)) {
                char *names = strdup(argv[2]), *save = NULL;
                int rc = 0;
                for (char *name = strtok_r(names, "+", &save); name != NULL && rc == 0; name = strtok_r(NULL, "+", &save)) {
                        rc = run_one(name, argc, argv);
                }
                free(names);
                fflush(stdout);
                return rc;
        }
        fprintf(stderr, "usage: %s list | run <name>[+<name>...] <options|-> <codec> <cf|pp> <tiles> <out prefix> <w> <h> <in.raw> [...]\n", argv[0]);
        return 1;
}
