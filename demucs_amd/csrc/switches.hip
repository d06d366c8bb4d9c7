// The engine's environment switches: the one place that reads the process environment (host code only, no kernel).
// Everything else asks switches(); the two run-time globals that start from the environment (g_transpose_tiles,
// g_istft_fused in fft.hip) take their initial value from it, so the environment is read when the library is loaded.
#include <cstdlib>

#include "common.h"
#include "kernels.h"

namespace mi {

static bool present(const char *name) { return getenv(name) != nullptr; }
// a number: `unset` when the variable is absent, else whether it parses to a non-zero value
static bool nonzero(const char *name, bool unset) {
    const char *e = getenv(name);
    return e ? atoi(e) != 0 : unset;
}

static Switches read_switches() {
    Switches s{};
    s.no_dma = present("MI_NO_DMA");
    s.no_dma_tap = present("MI_NO_DMA_TAP");
    s.no_dma_rows = present("MI_NO_DMA_ROWS");
    s.no_dma_dconv = present("MI_NO_DMA_DCONV");
    s.small_tile = nonzero("MI_SMALL_TILE", true);
    s.mgroups = present("MI_MGROUPS");
    const char *mode = getenv("MI_X6_MODE");
    s.x6_plain_only = mode && atoi(mode) == 1;
    s.img256 = nonzero("MI_IMG256", false);
    s.half_tile256 = nonzero("MI_HALF_TILE256", true);
    s.x6_scope = present("MI_X6") ? (nonzero("MI_X6", false) ? 2 : 0) : 1;
    s.no_tap_image = present("MI_NO_TAP_IMAGE");
    s.no_enc_image = present("MI_NO_ENC_IMAGE");
    s.no_dconv_time = present("MI_NO_DCONV_TIME");
    s.no_lin2_stats = present("MI_NO_LIN2_STATS");
    s.no_ffn_image = present("MI_NO_FFN_IMAGE");
    s.no_qkv_heads = present("MI_NO_QKV_HEADS");
    s.no_input_image = present("MI_NO_INPUT_IMAGE");
    s.one_stream = present("MI_ONE_STREAM");
    s.debug_sync = present("MI_DEBUG_SYNC");
    const char *prio = getenv("MI_SIDE_PRIO");
    s.side_prio = !prio ? 0 : prio[0] == 'l' ? -1 : 1;
    s.h_no_deep_tap = present("MI_H_NO_DEEP_TAP");
    s.h_no_last_tap = present("MI_H_NO_LAST_TAP");
    s.h_one_stream = present("MI_H_ONE_STREAM");
    s.lstm_steps = nonzero("MI_LSTM_STEPS", false);
    s.lstm_write_through = present("MI_LSTM_WRITE_THROUGH");
    s.lstm_debug = present("MI_LSTM_DEBUG");
    const char *tiles = getenv("MI_TRANSPOSE_TILES");
    s.transpose_tiles = !tiles ? 0 : atoi(tiles) > 1 ? (atoi(tiles) & 7) : 7;
    s.istft_split = present("MI_ISTFT_SPLIT");
    const char *row = getenv("MI_DCONV_ROW");
    s.dconv_row_lds = row && row[0] == 'l';
    return s;
}

const Switches &switches() {
    static const Switches s = read_switches();
    return s;
}

}  // namespace mi

// One NAME=value line per field, the value being the parsed meaning (include/demucs_amd.h)
extern "C" int mi_debug_switches(char *buf, int32_t n) {
    const mi::Switches &s = mi::switches();
    static const char *const scope[3] = {"none", "default", "all"}, *const prio[3] = {"low", "normal", "high"};
    const int len = snprintf(
        buf, buf && n > 0 ? (size_t)n : 0,
        "MI_NO_DMA=%d\nMI_NO_DMA_TAP=%d\nMI_NO_DMA_ROWS=%d\nMI_NO_DMA_DCONV=%d\nMI_SMALL_TILE=%d\nMI_MGROUPS=%d\nMI_X6_MODE=%d\nMI_X6=%s\n"
        "MI_NO_TAP_IMAGE=%d\nMI_NO_ENC_IMAGE=%d\nMI_NO_DCONV_TIME=%d\nMI_NO_LIN2_STATS=%d\nMI_NO_FFN_IMAGE=%d\nMI_NO_QKV_HEADS=%d\n"
        "MI_NO_INPUT_IMAGE=%d\nMI_ONE_STREAM=%d\nMI_DEBUG_SYNC=%d\nMI_SIDE_PRIO=%s\nMI_H_NO_DEEP_TAP=%d\nMI_H_NO_LAST_TAP=%d\n"
        "MI_H_ONE_STREAM=%d\nMI_LSTM_STEPS=%d\nMI_LSTM_WRITE_THROUGH=%d\nMI_LSTM_DEBUG=%d\nMI_TRANSPOSE_TILES=%d\nMI_ISTFT_SPLIT=%d\n"
        "MI_DCONV_ROW=%s\nMI_IMG256=%d\nMI_HALF_TILE256=%d\n",
        s.no_dma, s.no_dma_tap, s.no_dma_rows, s.no_dma_dconv, s.small_tile, s.mgroups, s.x6_plain_only, scope[s.x6_scope],
        s.no_tap_image, s.no_enc_image, s.no_dconv_time, s.no_lin2_stats, s.no_ffn_image, s.no_qkv_heads, s.no_input_image, s.one_stream,
        s.debug_sync, prio[s.side_prio + 1], s.h_no_deep_tap, s.h_no_last_tap, s.h_one_stream, s.lstm_steps, s.lstm_write_through,
        s.lstm_debug, s.transpose_tiles, s.istft_split, s.dconv_row_lds ? "lds" : "wave", s.img256, s.half_tile256);
    return len;
}
