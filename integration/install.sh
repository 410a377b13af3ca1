#!/bin/sh
# Puts the MI355X modules into an UltraGrid source tree and patches its configure.ac (integration/ultragrid_mi355x.patch):
#   sh integration/install.sh <ultragrid-source-dir>
# then, in that tree:  ./autogen.sh --with-ug-mi355x=<prefix holding lib/libug_mi355x.so> && make
# Files keep their content; only their names follow the reference's layout (src/video_compress/<name>.cpp -> ultragrid_vcompress_<name>.so).
# The module sources include the C ABI as "../../include/ug_mi355x.h": all the destination directories are two levels below the
# tree's root, so the header goes to <tree>/include/.
set -e
UG=${1:?usage: install.sh <ultragrid-source-dir>}
HERE=$(cd "$(dirname "$0")" && pwd); ROOT=$(dirname "$HERE"); M=$ROOT/ultragrid_amd/module
test -f "$UG/configure.ac" || { echo "$UG: no configure.ac there" >&2; exit 1; }
mkdir -p "$UG/include" "$UG/src/video_compress" "$UG/src/video_decompress" "$UG/src/libavcodec" "$UG/src/rtp" "$UG/src/vo_postprocess" "$UG/src/capture_filter"
cp "$ROOT/include/ug_mi355x.h"               "$UG/include/ug_mi355x.h"
cp "$M/vcompress_dxt_mi355x.cpp"             "$UG/src/video_compress/dxt_mi355x.cpp"
cp "$M/vcompress_jpeg_mi355x.cpp"            "$UG/src/video_compress/jpeg_mi355x.cpp"
cp "$M/vcompress_uyvy_mi355x.cpp"            "$UG/src/video_compress/uyvy_mi355x.cpp"
cp "$M/ug_codec_map.h" "$M/mi355x_frame_sharder.h" "$M/mi355x_tile_encoder.h" "$M/mi355x_hip_device.h" "$UG/src/video_compress/"
cp "$M/vdecompress_dxt_mi355x.c"             "$UG/src/video_decompress/dxt_mi355x.c"
cp "$M/vdecompress_jpeg_mi355x.c"            "$UG/src/video_decompress/jpeg_mi355x.c"
cp "$M/vdecompress_jpeg_to_dxt_mi355x.c"     "$UG/src/video_decompress/jpeg_to_dxt_mi355x.c"
cp "$M/mi355x_receiver.h" "$M/mi355x_gpu_state.h" "$UG/src/video_decompress/"
cp "$M/lavc_conv_mi355x.cpp"                 "$UG/src/libavcodec/lavc_conv_mi355x.cpp"
cp "$M/ldgm_gpu_mi355x.cpp"                  "$UG/src/rtp/ldgm_gpu_mi355x.cpp"
cp "$M/mi355x_receiver.h"                    "$UG/src/rtp/"
cp "$M/vo_pp_scale_mi355x.c"                "$UG/src/vo_postprocess/scale_mi355x.c"
cp "$M/vo_pp_deinterlace_mi355x.c"          "$UG/src/vo_postprocess/deinterlace_mi355x.c"
cp "$M/vo_pp_compose_mi355x.c"              "$UG/src/vo_postprocess/compose_mi355x.c"
cp "$M/mi355x_receiver.h" "$M/mi355x_gpu_state.h" "$M/ug_codec_map.h" "$UG/src/vo_postprocess/"
cp "$M/capture_filter_pixel_mi355x.c"       "$UG/src/capture_filter/pixel_mi355x.c"
cp "$M/mi355x_receiver.h" "$M/mi355x_gpu_state.h" "$M/ug_codec_map.h" "$UG/src/capture_filter/"
if grep -q "found_ug_mi355x" "$UG/configure.ac"; then
        echo "configure.ac is patched already"
else
        patch -p1 -d "$UG" < "$HERE/ultragrid_mi355x.patch"
fi
echo "installed into $UG: 6 modules, the scale and de-interlacing postprocessors, the colour / mirror filters, the composition filters, the lavc hook and the ldgm_gpu library; configure with --with-ug-mi355x=<prefix>"
