/**
 * @file ug_vopp_harness.c
 * The receiver's postprocess chain through UltraGrid's own framework: src/vo_postprocess.c + the lib_common registry, with the module object
 * vo_pp_scale_mi355x.o linked in (registration: a static constructor), built as a build without the reference's GL `scale` module
 * (MI355X_NO_SCALE_PP, what the configure patch defines there).
 *
 * usage: ug_vopp_harness list                      the VIDEO_POSTPROCESS names of the registry, one per line; "same=1" when load_library("scale")
 *                                                  and load_library("scale_mi355x") are the same module
 *        ug_vopp_harness run <cfg> <UYVY|RGBA> <prog|merged> <extra pitch bytes> <w> <h> <in.raw> <out.raw> [<w> <h> <in.raw> <out.raw> ...]
 *            vo_postprocess_init(cfg); per frame: vo_postprocess_reconfigure when the size changes (first frame included) -> get_out_desc ->
 *            getf -> the input bytes into it -> vo_postprocess(in, out, req_pitch = vc_get_linesize(out_w) + extra) into a frame pre-filled with
 *            0xA5 -> out.raw (req_pitch * out_h bytes); then vo_postprocess(NULL) (the flush) and vo_postprocess_done.
 *            stdout per frame: "frame <out_w> <out_h> <codec> <interlacing> <tile_count> <display mode> ret=<0|1>", then "null=<0|1>"
 * UG_PARAM=<k>=<v>[,...] answers get_commandline_param (e.g. mi355x-device=0); UG_VOPP_TILES=<n> sets the description's tile_count (default 1).  Exit 0 = all frames processed, 2 = init refused, 3 = reconfigure
 * refused, 4 = postprocess failed.
 */
#include <stdbool.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "debug.h"
#include "lib_common.h"
#include "types.h"
#include "video_codec.h"
#include "video_display.h"
#include "video_frame.h"
#include "vo_postprocess.h"

#define UG_HARNESS_NAME "ug_vopp_harness"
#include "ug_harness_host.h" /* what host.cpp would provide; get_commandline_param answers from UG_PARAM */

static int run(int argc, char **argv)
{
        const char *cfg = argv[2];
        const codec_t codec = strcmp(argv[3], "UYVY") == 0 ? UYVY : RGBA;
        const enum interlacing_t inter = strcmp(argv[4], "merged") == 0 ? INTERLACED_MERGED : PROGRESSIVE;
        const int extra = atoi(argv[5]);
        const unsigned tiles = getenv("UG_VOPP_TILES") ? (unsigned) atoi(getenv("UG_VOPP_TILES")) : 1u;
        struct vo_postprocess_state *s = vo_postprocess_init(cfg);
        if (s == NULL) {
                return 2;
        }
        struct video_desc cur = { 0 };
        struct video_frame *out = NULL;
        int pitch = 0, rc = 0;
        for (int a = 6; a + 3 < argc; a += 4) {
                const struct video_desc desc = { .width = (unsigned) atoi(argv[a]), .height = (unsigned) atoi(argv[a + 1]), .color_spec = codec,
                                                 .interlacing = inter, .fps = 25.0, .tile_count = tiles };
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
                pitch = vc_get_linesize(od.width, od.color_spec) + extra;
                const size_t out_len = (size_t) pitch * od.height;
                out->tiles[0].data = malloc(out_len);
                memset(out->tiles[0].data, 0xA5, out_len);
                struct video_frame *in = vo_postprocess_getf(s);
                FILE *f = fopen(argv[a + 2], "rb");
                const size_t n = f ? fread(in->tiles[0].data, 1, in->tiles[0].data_len, f) : 0;
                if (f) fclose(f);
                if (n != in->tiles[0].data_len) {
                        fprintf(stderr, "%s: %zu of %u bytes\n", argv[a + 2], n, in->tiles[0].data_len);
                        rc = 1;
                        break;
                }
                const bool ok = vo_postprocess(s, in, out, pitch);
                printf("frame %u %u %s %d %u %d ret=%d\n", od.width, od.height, get_codec_name(od.color_spec), (int) od.interlacing, od.tile_count, mode, (int) ok);
                f = fopen(argv[a + 3], "wb");
                if (!f || fwrite(out->tiles[0].data, 1, out_len, f) != out_len) {
                        perror(argv[a + 3]);
                        rc = 1;
                        break;
                }
                fclose(f);
                if (!ok) {
                        rc = 4;
                        break;
                }
        }
        if (rc == 0 && out) {
                printf("null=%d\n", (int) vo_postprocess(s, NULL, out, pitch));
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
                const void *a = load_library("scale", LIBRARY_CLASS_VIDEO_POSTPROCESS, VO_PP_ABI_VERSION);
                const void *b = load_library("scale_mi355x", LIBRARY_CLASS_VIDEO_POSTPROCESS, VO_PP_ABI_VERSION);
                printf("same=%d\n", a != NULL && a == b);
                return 0;
        }
        if (argc >= 10 && strcmp(argv[1], "run") == 0 && (argc - 6) % 4 == 0) {
                return run(argc, argv);
        }
        fprintf(stderr, "usage: %s list | run <cfg> <UYVY|RGBA> <prog|merged> <extra pitch> <w> <h> <in.raw> <out.raw> [...]\n", argv[0]);
        return 1;
}
