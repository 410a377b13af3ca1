/**
 * @file vcompress_uyvy_mi355x.cpp
 * UltraGrid video_compress module "uyvy_mi355x" (-c uyvy_mi355x[:dev=<n>[,<n>...]][:workers=<n>][:batch=<n>]) -- the GPU stand-in for the
 * reference's "RGB to UYVY compression" (src/video_compress/uyvy.cpp), backed by libug_mi355x.so (include/ug_mi355x.h, UG_PF_UYVY_GL).
 *
 * The reference converts RGB / RGBA frames with dxt_compress/rgba_to_yuv422.glsl in an OpenGL context and aborts where it cannot create one
 * (uyvy.cpp:133): on a headless server the sender dies.  This module computes the same shader on the GPU (ug_hip_pixfmt_convert to
 * UG_PF_UYVY_GL; the bytes and the two slips of the reference that are not reproduced: INTEGRATION.md, "-c uyvy").  In a build without the
 * reference's module (configure decided uyvy=no: MI355X_NO_UYVY_COMPRESS) it also takes the hidden name "uyvy", as a drop-in.
 *
 * Same shape as the other compress modules here: the asynchronous frame API on mi355x_frame_sharder.h (dev= / workers= / batch= are
 * consumed there), per-tile states with one HIP stream each, uploads and downloads on the device's copy lanes, output frames from a pinned
 * pool, device-resident input converted in place.  Input other than RGB / RGBA is refused with the reference's message (uyvy.cpp:158-168).
 */
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#ifdef HAVE_CONFIG_H
#include "config.h" // MI355X_NO_UYVY_COMPRESS (integration/ultragrid_mi355x.patch)
#endif
#include "debug.h"
#include "host.h"
#include "lib_common.h"
#include "types.h"
#include "utils/video_frame_pool.h"
#include "video_codec.h"
#include "video_compress.h"
#include "video_frame.h"

#include "../../include/ug_mi355x.h"
#include "mi355x_hip_device.h"

#define MOD_NAME "[UYVY MI355X] "

#define CHECK_HIP(cmd, msg, action) \
        if ((cmd) != UG_HIP_SUCCESS) { \
                MSG(ERROR, "%s: %s\n", msg, ug_hip_last_error_string()); \
                action; \
        }

namespace {

struct state_video_compress_uyvy_mi355x : mi355x::tile_encoder_state<mi355x::hip_device> {
        state_video_compress_uyvy_mi355x() : tile_encoder_state(MOD_NAME) {}
        ug_pixfmt_t       in_fmt = UG_PF_NONE;
        void             *dev_in = nullptr;  ///< uploaded frame
        void             *dev_out = nullptr; ///< UYVY
        size_t            in_len = 0, out_len = 0;
};

void usage()
{
        printf("MI355X RGB/RGBA to UYVY compression (the conversion of -c uyvy, without OpenGL):\n"
               "\t-c uyvy_mi355x[:dev=<index>[,<index>...]][:workers=<per device>][:batch=<frames>][:numa=<0|1>]\n"
               "\t\tdev  - HIP device index or list (default 0)\n");
}

void *uyvy_mi355x_compress_init(struct module *parent, const char *fmt)
{
        (void) parent;
        auto *s = new state_video_compress_uyvy_mi355x();
        for (const std::string &tok : mi355x::option_tokens(fmt)) {
                if (s->internal_option(tok)) { // (the worker's device; batch_slices= is taken and not used: there is no batch entry)
                } else if (tok == "help") {
                        usage();
                        delete s;
                        return INIT_NOERR;
                } else if (!tok.empty()) {
                        MSG(ERROR, "unknown option: %s\n", tok.c_str());
                        usage();
                        delete s;
                        return nullptr;
                }
        }
        return mi355x::opened(s);
}

bool configure_with(state_video_compress_uyvy_mi355x *s, struct video_desc desc)
{
        switch (desc.color_spec) { // uyvy.cpp:158-168
        case RGB: s->in_fmt = UG_PF_RGB; break;
        case RGBA: s->in_fmt = UG_PF_RGBA; break;
        default:
                fprintf(stderr, "[UYVY compress] We can transform only RGB or RGBA to UYVY.\n");
                return false;
        }
        s->in_len = (size_t) vc_get_linesize(desc.width, desc.color_spec) * desc.height;
        s->out_len = (size_t) vc_get_linesize(desc.width, UYVY) * desc.height;
        CHECK_HIP(s->buffers.get(&s->dev_in, s->in_len + MAX_PADDING), "Could not allocate device input buffer", return false);
        CHECK_HIP(s->buffers.get(&s->dev_out, s->out_len), "Could not allocate device output buffer", return false);
        struct video_desc compressed_desc = desc;
        compressed_desc.color_spec = UYVY;
        compressed_desc.tile_count = 1;
        s->pool->reconfigure(compressed_desc, s->out_len);
        return true;
}

std::shared_ptr<video_frame> uyvy_mi355x_compress_tile(void *state, std::shared_ptr<video_frame> tx)
{
        if (!tx) {
                return {}; // poison pill (video_compress.cpp:345-347)
        }
        auto *s = static_cast<state_video_compress_uyvy_mi355x *>(state);
        CHECK_HIP(ug_hip_set_device(s->device), "set device", return {}); // tile callbacks run on pool threads

        if (!mi355x::configured_for(s, tx.get(), configure_with)) {
                return {};
        }
        const int w = (int) tx->tiles[0].width, h = (int) tx->tiles[0].height;
        const void *src = mi355x::frame_source(s, *tx, s->dev_in, s->in_len, 1); // (the converter takes any alignment)
        if (src == nullptr) {
                return {};
        }
        CHECK_HIP(ug_hip_pixfmt_convert(s->in_fmt, UG_PF_UYVY_GL, src, s->dev_out, w, h, 0, 0, 0, 8, 16, s->stream), "conversion failed", return {});
        return mi355x::finished_frame(s, s->dev_out, s->out_len);
}

compress_module_info get_uyvy_mi355x_module_info()
{
        compress_module_info module_info;
        module_info.name = "uyvy_mi355x";
        return module_info;
}

const struct video_compress_info uyvy_mi355x_info = mi355x::sharded_compress_info(
        mi355x::hip_module_init<uyvy_mi355x_compress_init, uyvy_mi355x_compress_tile, mi355x::tile_done<state_video_compress_uyvy_mi355x>>, get_uyvy_mi355x_module_info);

REGISTER_MODULE(uyvy_mi355x, &uyvy_mi355x_info, LIBRARY_CLASS_VIDEO_COMPRESS, VIDEO_COMPRESS_ABI_VERSION);
// The reference registers "uyvy" (uyvy.cpp:288) where configure found OpenGL; in such a build nothing of its registry changes and this module
// is -c uyvy_mi355x.  Where configure left the GL module out (the patch's MI355X_NO_UYVY_COMPRESS), "-c uyvy" is this module.
#ifdef MI355X_NO_UYVY_COMPRESS
REGISTER_HIDDEN_MODULE(uyvy, &uyvy_mi355x_info, LIBRARY_CLASS_VIDEO_COMPRESS, VIDEO_COMPRESS_ABI_VERSION);
#endif

} // end of anonymous namespace
