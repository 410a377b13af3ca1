/**
 * @file ug_fake_compress.cpp
 * TEST-ONLY video_compress module "fake": the skeleton of vcompress_dxt_mi355x.cpp / vcompress_jpeg_mi355x.cpp (mi355x_tile_encoder.h: the state core,
 * the lazy reconfigure on a format change, the batch entry, the pool and the tail of a frame, behind mi355x::sharded_init with workers=, batch=, dev=
 * and the asynchronous frame API), with the GPU replaced by a hash, so that the run-time conventions
 * of the boundary (format change in flight, CHANGE_COMPRESS, compress_done with frames queued) can be driven through the reference's framework on a
 * CPU box, under ThreadSanitizer and AddressSanitizer (tests/test_runtime_conventions.py).  Never part of the product: it is linked into
 * oracle/_ref/ug_runtime_harness_fake* only.
 *
 * -c fake[:tag=<n>][:delay_us=<max>][:fail_every=<k>] + the sharder's options.  A "compressed" frame is 80 bytes:
 *   u32 magic 'FAKE', tag, cfg_w, cfg_h, cfg_codec, cfg_interlacing   <- what the state was CONFIGURED for when it encoded the frame
 *   u32 w, h, codec, interlacing                                      <- the frame's own desc
 *   u64 fnv1a(tile bytes), u32 batch_n, device, in_len, state_serial, pad[2]
 * so a frame of one format encoded under the configuration of another is visible in the output (cfg_* != own desc).
 */
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "debug.h"
#include "host.h"
#include "lib_common.h"
#include "types.h"
#include "utils/video_frame_pool.h"
#include "video_codec.h"
#include "video_compress.h"
#include "video_frame.h"

#include "mi355x_tile_encoder.h"

#define MOD_NAME "[fake] "

namespace {

constexpr size_t OUT_LEN = 80;
std::atomic<uint32_t> g_state_serial{0};
std::atomic<int> g_live_states{0}; // printed at exit: every init must have met its done

/// the device of this module: host memory, copies that are done when they return, no streams
struct fake_device {
        using stream_t = int;
        using frame_allocator = default_data_allocator;
        static int set_device(int d) { return d >= 0 && d < 64 ? 0 : -1; }
        static int stream_create(stream_t *stream) { *stream = 1; return 0; }
        static void stream_destroy(stream_t) {}
        static int stream_sync(stream_t) { return 0; }
        static int malloc(void **buf, size_t len) { return (*buf = ::malloc(len)) != nullptr ? 0 : -1; }
        static void free(void *buf) { ::free(buf); }
        static int download(int, void *dst, const void *src, size_t len, stream_t) { memcpy(dst, src, len); return 0; }
        static const char *last_error() { return "no such fake device"; }
};

struct state_fake : mi355x::tile_encoder_state<fake_device> {
        state_fake() : tile_encoder_state(MOD_NAME) {}
        struct video_desc cfg_desc{};
        uint32_t tag = 0;
        unsigned delay_us = 0, fail_every = 0;
        uint32_t serial = 0;
        uint64_t encoded = 0;
        std::mt19937 rng{1};
        void *dev_in = nullptr; // stands for the device buffers: sized by configure_with(), so a stale size is an out-of-bounds write ASan sees
};

void *fake_init(struct module *, const char *fmt)
{
        auto *s = new state_fake();
        for (const std::string &tok : mi355x::option_tokens(fmt)) {
                if (tok.rfind("tag=", 0) == 0) s->tag = (uint32_t) atoi(tok.c_str() + 4);
                else if (tok.rfind("delay_us=", 0) == 0) s->delay_us = (unsigned) atoi(tok.c_str() + 9);
                else if (tok.rfind("fail_every=", 0) == 0) s->fail_every = (unsigned) atoi(tok.c_str() + 11);
                else if (s->internal_option(tok)) continue;
                else if (tok == "help") { printf("fake compress: test only\n"); delete s; return INIT_NOERR; }
                else if (!tok.empty()) { MSG(ERROR, "unknown option: %s\n", tok.c_str()); delete s; return nullptr; }
        }
        s->serial = g_state_serial++;
        s->rng.seed(s->serial * 7919u + 13u);
        void *state = mi355x::opened(s);
        if (state != nullptr) g_live_states++;
        return state;
}

bool configure_with(state_fake *s, struct video_desc desc)
{
        if (desc.width % 4 != 0 || desc.height % 4 != 0) {
                MSG(ERROR, "Frame size %ux%u is not a multiple of the 4x4 block\n", desc.width, desc.height);
                return false;
        }
        s->cfg_desc = desc;
        if (s->buffers.get(&s->dev_in, (size_t) vc_get_linesize(desc.width, desc.color_spec) * desc.height) != 0) return false;
        struct video_desc out = desc;
        out.color_spec = DXT1;
        out.tile_count = 1;
        s->pool->reconfigure(out, OUT_LEN);
        return true;
}

uint64_t fnv1a(const char *p, size_t n)
{
        uint64_t h = 1469598103934665603ull;
        for (size_t i = 0; i < n; i++) { h ^= (unsigned char) p[i]; h *= 1099511628211ull; }
        return h;
}

std::shared_ptr<video_frame> encode_configured(state_fake *s, const std::shared_ptr<video_frame> &tx, uint32_t batch_n)
{
        if (s->delay_us) std::this_thread::sleep_for(std::chrono::microseconds(s->rng() % (s->delay_us + 1)));
        s->encoded++;
        if (s->fail_every && s->encoded % s->fail_every == 0) return {};
        memcpy(s->dev_in, tx->tiles[0].data, tx->tiles[0].data_len); // the "upload": into the buffer the CONFIGURED geometry sized
        const struct video_desc d = video_desc_from_frame(tx.get());
        uint32_t rec[20] = { 0x454b4146u, s->tag, s->cfg_desc.width, s->cfg_desc.height, (uint32_t) s->cfg_desc.color_spec, (uint32_t) s->cfg_desc.interlacing,
                             d.width, d.height, (uint32_t) d.color_spec, (uint32_t) d.interlacing };
        const uint64_t h = fnv1a((const char *) s->dev_in, tx->tiles[0].data_len);
        memcpy(&rec[10], &h, 8);
        rec[12] = batch_n; rec[13] = (uint32_t) s->device; rec[14] = tx->tiles[0].data_len; rec[15] = s->serial;
        return mi355x::finished_frame(s, rec, OUT_LEN); // the "download" into a frame of the pool
}

std::shared_ptr<video_frame> fake_compress_tile(void *state, std::shared_ptr<video_frame> tx)
{
        if (!tx) return {};
        auto *s = static_cast<state_fake *>(state);
        if (!mi355x::configured_for(s, tx.get(), configure_with)) return {};
        return encode_configured(s, tx, 1);
}

bool no_batch_slices(state_fake *) { return true; }

void encode_batch(state_fake *s, const mi355x::frames_t &in, mi355x::frames_t &out)
{
        for (size_t i = 0; i < in.size(); i++) out[i] = encode_configured(s, in[i], (uint32_t) in.size());
}

mi355x::frames_t fake_compress_batch(void *state, mi355x::frames_t in)
{
        return mi355x::compress_batch(static_cast<state_fake *>(state), std::move(in), fake_compress_tile, no_batch_slices, encode_batch);
}

void fake_done(void *state)
{
        g_live_states--;
        mi355x::tile_done<state_fake>(state);
}

void *fake_module_init(struct module *parent, const char *cfg)
{
        return mi355x::sharded_init(parent, cfg, fake_init, fake_compress_tile, fake_done, fake_device::set_device, fake_compress_batch);
}

compress_module_info get_fake_module_info()
{
        compress_module_info mi;
        mi.name = "fake";
        return mi;
}

const struct video_compress_info fake_info = mi355x::sharded_compress_info(fake_module_init, get_fake_module_info);
REGISTER_MODULE(fake, &fake_info, LIBRARY_CLASS_VIDEO_COMPRESS, VIDEO_COMPRESS_ABI_VERSION);

struct report_at_exit {
        ~report_at_exit() { printf("FAKE live_states=%d created=%u\n", g_live_states.load(), g_state_serial.load()); }
} g_report;

} // namespace
