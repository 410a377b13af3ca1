/**
 * @file mi355x_gpu_state.h
 * The GPU half of a module state, shared by the plain-C MI355X modules (vo_pp_scale, vo_pp_deinterlace, capture_filter_pixel, vo_pp_compose,
 * vdecompress_dxt): the device the state runs on with its stream, and buffers that follow the frame.  Plain C.
 *
 * A call into a module goes: mi355x_gpu_enter -> (mi355x_buf_reserve) -> queue copies and kernels on g->stream -> mi355x_gpu_finish, which
 * synchronises the stream whatever happened before: nothing asynchronous is left pending when the call returns, also on failure (the caller
 * reuses its frames).  The module's message prefix is handed over once, at open.
 */
#ifndef MI355X_GPU_STATE_H
#define MI355X_GPU_STATE_H

#include "mi355x_receiver.h"

struct mi355x_gpu {
        const char     *mod_name;
        int             device; ///< --param mi355x-device / -D (mi355x_receiver.h)
        ug_hip_stream_t stream; ///< NULL: never opened, or closed
};

/** the device becomes the calling thread's; false (and a message) when it cannot */
static inline bool mi355x_gpu_enter(const struct mi355x_gpu *g)
{
        if (ug_hip_set_device(g->device) != UG_HIP_SUCCESS) {
                log_msg(LOG_LEVEL_ERROR, "%scannot use HIP device %d: %s\n", g->mod_name, g->device, ug_hip_last_error_string());
                return false;
        }
        return true;
}

/** the states of a module take the listed devices in turn (`state_counter`); on false g->stream == NULL and something has been said */
static inline bool mi355x_gpu_open(struct mi355x_gpu *g, unsigned *state_counter, const char *mod_name)
{
        g->mod_name = mod_name;
        g->stream = NULL;
        g->device = mi355x_next_state_device(state_counter, mod_name);
        if (g->device < 0) {
                return false;
        }
        if (ug_hip_set_device(g->device) != UG_HIP_SUCCESS || ug_hip_stream_create(&g->stream) != UG_HIP_SUCCESS) {
                log_msg(LOG_LEVEL_ERROR, "%scannot use HIP device %d: %s\n", mod_name, g->device, ug_hip_last_error_string());
                g->stream = NULL;
                return false;
        }
        return true;
}

/** the end of a call: says "<what> failed" for !ok (what == NULL: the caller has spoken), then waits for whatever was queued; @returns ok && synced */
static inline bool mi355x_gpu_finish(const struct mi355x_gpu *g, bool ok, const char *what)
{
        if (!ok && what != NULL) log_msg(LOG_LEVEL_ERROR, "%s%s failed: %s\n", g->mod_name, what, ug_hip_last_error_string());
        const bool synced = ug_hip_stream_sync(g->stream) == UG_HIP_SUCCESS;
        if (ok && !synced) log_msg(LOG_LEVEL_ERROR, "%sstream sync failed: %s\n", g->mod_name, ug_hip_last_error_string());
        return ok && synced;
}

/** waits for the stream and destroys it; nothing on a state that was never opened.  Frees no buffers: the caller releases them, before this or
 * after it (the device stays the current one) */
static inline void mi355x_gpu_close(struct mi355x_gpu *g)
{
        if (g->stream == NULL) {
                return;
        }
        ug_hip_set_device(g->device);
        ug_hip_stream_sync(g->stream);
        ug_hip_stream_destroy(g->stream);
        g->stream = NULL;
}

struct mi355x_buf {
        void  *ptr;
        size_t cap;
        bool   pinned; ///< pinned host memory, not device memory
};

/** safe on an empty buf; the device of the state is the current one */
static inline void mi355x_buf_release(struct mi355x_buf *b)
{
        if (b->ptr != NULL) {
                if (b->pinned) ug_hip_free_host(b->ptr); else ug_hip_free(b->ptr);
        }
        b->ptr = NULL;
        b->cap = 0;
}

/** at least `len` bytes, grow-only: what is large enough stays.  Says nothing; after a failure the buf is empty */
static inline bool mi355x_buf_reserve(struct mi355x_buf *b, size_t len)
{
        if (len <= b->cap) {
                return true;
        }
        mi355x_buf_release(b);
        if ((b->pinned ? ug_hip_malloc_host(&b->ptr, len) : ug_hip_malloc(&b->ptr, len)) != UG_HIP_SUCCESS) {
                b->ptr = NULL;
                return false;
        }
        b->cap = len;
        return true;
}

#endif /* MI355X_GPU_STATE_H */
