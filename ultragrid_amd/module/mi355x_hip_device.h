/**
 * @file mi355x_hip_device.h
 * The device of the product's tile encoders (mi355x_tile_encoder.h): HIP through the kernel library's C ABI (include/ug_mi355x.h), and the
 * module_init that puts such an encoder on the frame sharder.
 */
#ifndef MI355X_HIP_DEVICE_H
#define MI355X_HIP_DEVICE_H

#include "../../include/ug_mi355x.h"
#include "mi355x_tile_encoder.h"

namespace mi355x {

struct hip_device {
        using stream_t = ug_hip_stream_t;
        /// pinned host memory for the compressed output frames (cuda_dxt.cpp:68-83 does the same with CUDA)
        struct frame_allocator : public video_frame_pool_allocator {
                void *allocate(size_t size) override {
                        void *ptr = nullptr;
                        return ug_hip_malloc_host(&ptr, size) == UG_HIP_SUCCESS ? ptr : nullptr;
                }
                void deallocate(void *ptr) override { ug_hip_free_host(ptr); }
                video_frame_pool_allocator *clone() const override { return new frame_allocator(*this); }
        };
        static int set_device(int device) { return ug_hip_set_device(device); } // tile callbacks run on pool threads
        static int stream_create(stream_t *stream) { return ug_hip_stream_create(stream); }
        static void stream_destroy(stream_t stream) { ug_hip_stream_destroy(stream); }
        static int stream_sync(stream_t stream) { return ug_hip_stream_sync(stream); }
        static int malloc(void **buf, size_t len) { return ug_hip_malloc(buf, len); }
        static void free(void *buf) { ug_hip_free(buf); }
        static int pointer_device(const void *ptr) { return ug_hip_pointer_device(ptr); }
        static bool pointer_is_device(const void *ptr) { return ug_hip_pointer_is_device(ptr); }
        static int upload(int device, void *dst, const void *src, size_t len, bool from_device, stream_t then_stream)
        {
                return ug_hip_upload_ordered(device, dst, src, len, from_device ? UG_HIP_MEMCPY_DEVICE_TO_DEVICE : UG_HIP_MEMCPY_HOST_TO_DEVICE, then_stream);
        }
        static int download(int device, void *dst, const void *src, size_t len, stream_t after_stream) { return ug_hip_download_ordered(device, dst, src, len, after_stream); }
        static const char *last_error() { return ug_hip_last_error_string(); }
};

/// module-level init: consumes dev=<list>, creates one worker (thread + per-tile encoder states) per listed device
template <tile_init_t init, tile_compress_t tile, tile_done_t done, tile_compress_batch_t batch = nullptr>
void *hip_module_init(struct module *parent, const char *cfg)
{
        return sharded_init(parent, cfg, init, tile, done, ug_hip_set_device, batch, ug_hip_bind_thread_to_device, ug_hip_device_numa_node);
}

} // namespace mi355x
#endif
