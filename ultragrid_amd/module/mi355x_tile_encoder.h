/**
 * @file mi355x_tile_encoder.h
 * What every tile encoder on mi355x_frame_sharder.h (init / compress_tile / compress_batch / done, one state per tile and worker) has between the
 * sharder and its own kernels: the state core with its stream, its device buffers and its pool of output frames, the lazy reconfigure on a format
 * change (cuda_dxt.cpp:196-204), where a frame is read from, how a result leaves, and the batch entry.  A module keeps its options, its
 * configure_with() and the kernel sequence of one frame and of one batch.
 *
 * Nothing here names the kernel library: the device is the policy type D (mi355x_hip_device.h for the product; the test-only module
 * ug_fake_compress.cpp runs this same code on host memory, under ThreadSanitizer and AddressSanitizer).  Messages take the module's prefix from
 * the state -- several modules are linked into one program, so shared code cannot use MSG() / MOD_NAME.
 */
#ifndef MI355X_TILE_ENCODER_H
#define MI355X_TILE_ENCODER_H

#include <cstdint>

#include "mi355x_frame_sharder.h"
#include "video_codec.h"
#include "video_compress.h"

namespace mi355x {

using frames_t = std::vector<std::shared_ptr<video_frame>>;

/// one buffer cut into equal slices, one per frame of a batch; the stride is a multiple of 16 so that every slice is as aligned as the base
struct slices {
        char  *base = nullptr;
        size_t stride = 0;
        char  *operator[](int f) const { return base + (size_t) f * stride; }
};

/// owns device memory: what get() handed out stays valid until release() (or the end of the owner), which frees all of it
template <class D> class device_buffers {
public:
        device_buffers() = default;
        device_buffers(const device_buffers &) = delete;
        device_buffers &operator=(const device_buffers &) = delete;
        ~device_buffers() { release(); }
        bool empty() const { return m_held.empty(); }
        /// as D::malloc: 0 on success
        int get(void **buf, size_t len)
        {
                const int rc = D::malloc(buf, len);
                if (rc == 0) m_held.push_back(*buf);
                return rc;
        }
        int get(slices *s, size_t slice_len, int count)
        {
                s->stride = (slice_len + 15) / 16 * 16;
                return get((void **) &s->base, s->stride * (size_t) count);
        }
        void release()
        {
                for (void *p : m_held) D::free(p);
                m_held.clear();
        }
private:
        std::vector<void *> m_held;
};

/// The core of a tile encoder's state; a module derives its state from it.  The destructor expects the state's device to be current (tile_done).
template <class D> struct tile_encoder_state {
        using device_t = D;
        const char *const    log_prefix; ///< the module's MOD_NAME
        struct video_desc    saved_desc{};
        int                  device = 0;
        typename D::stream_t stream{};
        /// slices of the batch buffers = the module's batch=<n>, handed down by the sharder as batch_slices=<n>; 16 if a caller hands batches to a state directly
        int                  batch_slices = 16;
        device_buffers<D>    buffers;       ///< of the configured geometry; released by the next reconfigure
        device_buffers<D>    batch_buffers; ///< the same once per frame of a batch: filled by the first batch after a reconfigure, released with `buffers`
        std::shared_ptr<video_frame_pool> pool = std::make_shared<video_frame_pool>(0, typename D::frame_allocator()); ///< shared with the frames it gives out (get_frame_keeping_pool)

        explicit tile_encoder_state(const char *mod_name) : log_prefix(mod_name) {}
        ~tile_encoder_state()
        {
                buffers.release();
                batch_buffers.release();
                if (stream) D::stream_destroy(stream);
        }

        /// the tokens mi355x::sharded_init appends for the tile init: dev=<n> of the worker, batch_slices=<n> when batching
        bool internal_option(const std::string &tok)
        {
                if (strncasecmp(tok.c_str(), "dev=", 4) == 0) {
                        device = atoi(tok.c_str() + 4);
                } else if (strncasecmp(tok.c_str(), "batch_slices=", 13) == 0) {
                        batch_slices = atoi(tok.c_str() + 13);
                        if (batch_slices < 1 || batch_slices > 16) batch_slices = 16;
                } else {
                        return false;
                }
                return true;
        }
};

/// the end of a tile init: the state with its device set and its stream created, or nullptr (said, and the state deleted)
template <class S> void *opened(S *s)
{
        using D = typename S::device_t;
        if (D::set_device(s->device) == 0 && D::stream_create(&s->stream) == 0) {
                return s;
        }
        log_msg(LOG_LEVEL_ERROR, "%scannot use HIP device %d: %s\n", s->log_prefix, s->device, D::last_error());
        delete s;
        return nullptr;
}

template <class S> void tile_done(void *state)
{
        auto *s = static_cast<S *>(state);
        S::device_t::set_device(s->device);
        delete s;
}

/// lazy reconfigure: true if the state is (now) configured for frames like `tx`; configure_with(s, desc) finds the buffers of the previous geometry released
template <class S, class F> bool configured_for(S *s, video_frame *tx, F configure_with)
{
        const struct video_desc desc = video_desc_from_frame(tx);
        if (video_desc_eq_excl_param(desc, s->saved_desc, PARAM_TILE_COUNT)) {
                return true;
        }
        s->buffers.release();
        s->batch_buffers.release();
        if (configure_with(s, desc)) {
                s->saved_desc = desc;
                return true;
        }
        log_msg(LOG_LEVEL_ERROR, "%sReconfiguration failed!\n", s->log_prefix);
        s->saved_desc = {};
        return false;
}

/// device-resident frame: mem_location == CUDA_MEM (types.h:295-298); the tile fan-out of video_compress.cpp drops that flag, so the pointer itself is asked as well
template <class D> bool on_device(const video_frame &tx)
{
        return tx.mem_location == CUDA_MEM || D::pointer_is_device(tx.tiles[0].data);
}

/// ordered upload of the frame's `len` bytes to `dst`, from host or from device memory; false: failed (said)
template <class S> bool upload_frame(S *s, const video_frame &tx, void *dst, size_t len)
{
        using D = typename S::device_t;
        if (D::upload(s->device, dst, tx.tiles[0].data, len, on_device<D>(tx), s->stream) == 0) {
                return true;
        }
        log_msg(LOG_LEVEL_ERROR, "%supload failed: %s\n", s->log_prefix, D::last_error());
        return false;
}

/// Where the kernels read the frame from.  A frame that lives on THIS state's device, `align`-byte aligned, is used in place, without an upload
/// (gpujpeg.cpp:617-622 does the same) -- unless the caller will write to its source (may_use_in_place = false).  With dev=<list> / several workers a
/// frame can reach a worker of another device, whose kernels must not dereference foreign memory: that one is copied over (peer copy), as host frames
/// are uploaded, to `staging`.  nullptr: the upload failed (said).
template <class S> const void *frame_source(S *s, const video_frame &tx, void *staging, size_t len, uintptr_t align, bool may_use_in_place = true)
{
        const char *data = tx.tiles[0].data;
        if (may_use_in_place && S::device_t::pointer_device(data) == s->device && ((uintptr_t) data & (align - 1)) == 0) {
                return data;
        }
        return upload_frame(s, tx, staging, len) ? staging : nullptr;
}

/// a frame of the state's pool with the ordered download of `len` result bytes queued behind the state's stream; {}: failed (said)
template <class S> std::shared_ptr<video_frame> download_frame(S *s, const void *result_dev, size_t len)
{
        using D = typename S::device_t;
        std::shared_ptr<video_frame> out = get_frame_keeping_pool(s->pool);
        if (D::download(s->device, out->tiles[0].data, result_dev, len, s->stream) != 0) {
                log_msg(LOG_LEVEL_ERROR, "%sD2H copy failed: %s\n", s->log_prefix, D::last_error());
                return {};
        }
        out->tiles[0].data_len = (unsigned int) len;
        return out;
}

/// the tail of a frame: download_frame and the one synchronisation of the tile
template <class S> std::shared_ptr<video_frame> finished_frame(S *s, const void *result_dev, size_t len, const char *sync_failed = "stream sync failed")
{
        using D = typename S::device_t;
        std::shared_ptr<video_frame> out = download_frame(s, result_dev, len);
        if (out && D::stream_sync(s->stream) != 0) {
                log_msg(LOG_LEVEL_ERROR, "%s%s: %s\n", s->log_prefix, sync_failed, D::last_error());
                return {};
        }
        return out;
}

/// The batch entry.  Fewer than two frames, more than there are slices, or a geometry the state is not configured for (the first frame of a new
/// one configures it on the way): one by one through `tile`.  Otherwise alloc_slices(s) fills s->batch_buffers on the first batch after a reconfigure
/// (false = no memory: what it got is released, one by one) and encode(s, in, out) does the batch; a result it leaves empty is a frame that failed.
template <class S> frames_t compress_batch(S *s, frames_t in, tile_compress_t tile, bool (*alloc_slices)(S *), void (*encode)(S *, const frames_t &in, frames_t &out))
{
        using D = typename S::device_t;
        frames_t out(in.size());
        bool batch = in.size() >= 2 && (int) in.size() <= s->batch_slices && D::set_device(s->device) == 0 &&
                     video_desc_eq_excl_param(video_desc_from_frame(in[0].get()), s->saved_desc, PARAM_TILE_COUNT);
        if (batch && s->batch_buffers.empty() && !alloc_slices(s)) {
                log_msg(LOG_LEVEL_WARNING, "%sno device memory for the batch buffers (%s): frames are encoded one by one\n", s->log_prefix, D::last_error());
                s->batch_buffers.release();
                batch = false;
        }
        if (batch) {
                encode(s, in, out);
        } else {
                for (size_t i = 0; i < in.size(); i++) out[i] = tile(s, std::move(in[i]));
        }
        return out;
}

/// the video_compress_info of a module on the sharder: the asynchronous frame API -- frames are dealt to one worker per listed GPU and popped in order
constexpr video_compress_info sharded_compress_info(compress_init_t module_init, compress_module_info (*get_module_info)())
{
        return { module_init, sharded_done, NULL, NULL, sharded_push, sharded_pop, NULL, NULL, get_module_info };
}

} // namespace mi355x
#endif
