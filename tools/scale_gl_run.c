/* scale_gl_run.c -- executes UltraGrid's `scale` video postprocessor (src/vo_postprocess/scale.c, compiled unmodified next to this file by
 * tests/golden/make_scale_gl_golden.py) on Mesa llvmpipe, headless, to pin the arithmetic GL leaves to the implementation (subtexel precision
 * and rounding of GL_LINEAR).  TEST INFRASTRUCTURE ONLY.
 *
 * What the module needs from the rest of UltraGrid is provided here:
 *   register_library         keeps the vo_postprocess_info the module registers (REGISTER_MODULE, lib_common.h)
 *   init_gl_context / gl_context_make_current / destroy_gl_context   a GL compatibility context from Mesa's software rasteriser loaded
 *                            through the DRI swrast interface (as oracle/glsl_ref.c makes one): no X server, no EGL, no GLEW
 *   vf_alloc / vf_get_tile / vf_free, vc_get_linesize   (video_frame.c, video_codec.c) for the two codecs the module takes
 * The GL entry points come through tools/scale_gl_shim/GL/glew.h.
 *
 * usage: scale_gl_run <UYVY|RGBA> <w> <h> <prog|merged> <out_w> <out_h> <req_pitch> <in.raw> <out.raw> [tiles]
 *   in.raw   tile_count x (vc_get_linesize(w) * h) bytes, copied into the frame getf returns
 *   out.raw  req_pitch * out_h bytes of the output tile, pre-filled with 0xA5 (what the module did not write keeps it)
 *   tiles    (default 1) the input description's tile_count; the output frame has ONE tile (get_out_desc says so) -- the module's loop
 *            writes out->tiles[i] for every input tile: here slot i > 0 points at a spare buffer, and "spare_written=<n>" reports its bytes
 *            that changed
 * stdout: "out <w> <h> <codec> <interlacing> <tile_count> <display_mode> ret=<postprocess return> null=<postprocess(NULL) return>"
 */
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "GL/glew.h"
#include <GL/internal/dri_interface.h>

#include "gl_context.h"
#include "lib_common.h"
#include "types.h"
#include "video_codec.h"
#include "video_display.h"
#include "video_frame.h"
#include "vo_postprocess.h"

#define SCALE_GL_DEFINE(name) __typeof__(name) p_##name; /* (name is p_name here: the type of the pointer the shim declared) */
SCALE_GL_FUNCS(SCALE_GL_DEFINE)

static const struct vo_postprocess_info *registered;

void register_library(const char *name, const void *info, enum library_class cls, int abi_version, enum mod_visibility_flag visibility)
{
        (void) visibility;
        if (strcmp(name, "scale") == 0 && cls == LIBRARY_CLASS_VIDEO_POSTPROCESS && abi_version == VO_PP_ABI_VERSION) {
                registered = info;
        }
}

int vc_get_linesize(unsigned int width, codec_t codec)
{
        return codec == UYVY ? (int) ((width + 1) / 2 * 4) : (int) (width * 4); /* codec_info[]: UYVY 2 px / 4 B, RGBA 1 px / 4 B */
}

struct video_frame *vf_alloc(int count)
{
        struct video_frame *f = calloc(1, sizeof *f + (size_t) count * sizeof(struct tile));
        f->tile_count = (unsigned) count;
        return f;
}

struct tile *vf_get_tile(struct video_frame *buf, int pos)
{
        return &buf->tiles[pos];
}

void vf_free(struct video_frame *buf)
{
        free(buf);
}

static void get_drawable_info(__DRIdrawable *d, int *x, int *y, int *w, int *h, void *p) { (void) d; (void) p; *x = *y = 0; *w = *h = 16; }
static void put_image(__DRIdrawable *d, int op, int x, int y, int w, int h, char *data, void *p) { (void) d; (void) op; (void) x; (void) y; (void) w; (void) h; (void) data; (void) p; }
static void get_image(__DRIdrawable *d, int x, int y, int w, int h, char *data, void *p) { (void) d; (void) x; (void) y; (void) p; memset(data, 0, (size_t) w * h * 4); }
static const __DRIswrastLoaderExtension swrast_loader = { .base = { __DRI_SWRAST_LOADER, 1 }, .getDrawableInfo = get_drawable_info, .putImage = put_image, .getImage = get_image };
static const __DRIextension *loader_exts[] = { &swrast_loader.base, NULL };

bool init_gl_context(struct gl_context *context, int which)
{
        (void) which; /* GL_CONTEXT_LEGACY: the compatibility API below */
        void *h = dlopen("/usr/lib/x86_64-linux-gnu/dri/swrast_dri.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("swrast_dri.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) { fprintf(stderr, "swrast_dri.so: %s\n", dlerror()); exit(2); }
        const __DRIextension **(*get_ext)(void) = (const __DRIextension **(*)(void)) dlsym(h, "__driDriverGetExtensions_swrast");
        if (!get_ext) { fprintf(stderr, "no __driDriverGetExtensions_swrast\n"); exit(2); }
        const __DRIextension **exts = get_ext();
        const __DRIcoreExtension *core = NULL;
        const __DRIswrastExtension *sw = NULL;
        for (int i = 0; exts[i]; i++) {
                if (!strcmp(exts[i]->name, __DRI_CORE)) core = (const __DRIcoreExtension *) exts[i];
                if (!strcmp(exts[i]->name, __DRI_SWRAST)) sw = (const __DRIswrastExtension *) exts[i];
        }
        if (!core || !sw || sw->base.version < 4) { fprintf(stderr, "DRI core / swrast(v4) extension missing\n"); exit(2); }
        const __DRIconfig **configs = NULL;
        __DRIscreen *scr = sw->createNewScreen2(0, loader_exts, exts, &configs, NULL);
        if (!scr || !configs || !configs[0]) { fprintf(stderr, "createNewScreen2 failed\n"); exit(2); }
        unsigned err = 0;
        __DRIcontext *ctx = sw->createContextAttribs(scr, __DRI_API_OPENGL, configs[0], NULL, 0, NULL, &err, NULL);
        __DRIdrawable *dr = ctx ? sw->createNewDrawable(scr, configs[0], NULL) : NULL;
        if (!ctx || !dr || !core->bindContext(ctx, dr, dr)) { fprintf(stderr, "context creation failed (err %u)\n", err); exit(2); }
        void *glapi = dlopen("libglapi.so.0", RTLD_NOW | RTLD_GLOBAL);
        void *(*gpa)(const char *) = glapi ? (void *(*)(const char *)) dlsym(glapi, "_glapi_get_proc_address") : NULL;
        if (!gpa) { fprintf(stderr, "libglapi: no _glapi_get_proc_address\n"); exit(2); }
#define SCALE_GL_LOAD(name) if (!(*(void **) &p_##name = gpa(#name))) { fprintf(stderr, "missing %s\n", #name); exit(2); }
        SCALE_GL_FUNCS(SCALE_GL_LOAD)
        context->legacy = 1;
        context->context = ctx;
        context->gl_major = 2;
        context->gl_minor = 1;
        return true;
}

void gl_context_make_current(struct gl_context *context)
{
        (void) context; /* one context, current since init_gl_context */
}

void destroy_gl_context(struct gl_context *context)
{
        (void) context;
}

int main(int argc, char **argv)
{
        if (argc != 10 && argc != 11) {
                fprintf(stderr, "usage: %s <UYVY|RGBA> <w> <h> <prog|merged> <out_w> <out_h> <req_pitch> <in.raw> <out.raw> [tiles]\n", argv[0]);
                return 1;
        }
        const codec_t codec = strcmp(argv[1], "UYVY") == 0 ? UYVY : RGBA;
        const int w = atoi(argv[2]), h = atoi(argv[3]), ow = atoi(argv[5]), oh = atoi(argv[6]), req_pitch = atoi(argv[7]);
        const int tiles = argc == 11 ? atoi(argv[10]) : 1;
        if (registered == NULL) { fprintf(stderr, "scale did not register\n"); return 2; }
        char cfg[64];
        snprintf(cfg, sizeof cfg, "%d:%d", ow, oh);
        void *st = registered->init(cfg);
        if (st == NULL) { fprintf(stderr, "init refused\n"); return 3; }
        struct video_desc desc = { .width = (unsigned) w, .height = (unsigned) h, .color_spec = codec, .fps = 25.0,
                                   .interlacing = strcmp(argv[4], "merged") == 0 ? INTERLACED_MERGED : PROGRESSIVE, .tile_count = (unsigned) tiles };
        if (!registered->reconfigure(st, desc)) { fprintf(stderr, "reconfigure refused\n"); return 3; }
        struct video_frame *in = registered->getf(st);
        FILE *f = fopen(argv[8], "rb");
        for (int i = 0; i < tiles; i++) {
                if (!f || fread(in->tiles[i].data, 1, in->tiles[i].data_len, f) != in->tiles[i].data_len) { fprintf(stderr, "short input\n"); return 1; }
        }
        fclose(f);
        struct video_desc od;
        int mode = -1;
        registered->get_out_desc(st, &od, &mode);
        const size_t out_len = (size_t) req_pitch * (size_t) oh;
        struct video_frame *out = vf_alloc(tiles);
        out->tile_count = 1;
        out->color_spec = od.color_spec;
        out->interlacing = od.interlacing;
        const size_t spare_len = out_len + 4096;
        for (int i = 0; i < tiles; i++) {
                out->tiles[i].width = od.width;
                out->tiles[i].height = od.height;
                out->tiles[i].data = malloc(i == 0 ? out_len + 4096 : spare_len); /* (+ what GL writes past a sheared read-back) */
                memset(out->tiles[i].data, 0xA5, i == 0 ? out_len + 4096 : spare_len);
                out->tiles[i].data_len = (unsigned) out_len;
        }
        const bool ret = registered->vo_postprocess(st, in, out, req_pitch);
        const bool null_ret = registered->vo_postprocess(st, NULL, out, req_pitch);
        p_glFinish();
        size_t spare_written = 0;
        for (int i = 1; i < tiles; i++) {
                for (size_t k = 0; k < spare_len; k++) spare_written += (uint8_t) out->tiles[i].data[k] != 0xA5;
        }
        printf("out %u %u %s %d %u %d ret=%d null=%d spare_written=%zu renderer=%s\n", od.width, od.height, od.color_spec == UYVY ? "UYVY" : "RGBA",
               (int) od.interlacing, od.tile_count, mode, (int) ret, (int) null_ret, spare_written, (const char *) p_glGetString(GL_RENDERER));
        f = fopen(argv[9], "wb");
        if (!f || fwrite(out->tiles[0].data, 1, out_len, f) != out_len) { perror(argv[9]); return 1; }
        fclose(f);
        registered->done(st);
        return 0;
}
