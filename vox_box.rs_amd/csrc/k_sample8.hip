// k_sample8.hip -- the 8-bit sample formats (VBX_SAMPLE_U8 / ULAW / ALAW: one byte per sample) of the two kernel
// templates whose other five formats live in units that count their kernels: session_ingest_all_<fmt> (vbx_session_ingest_all.hpp,
// k_session_channels.hip) and clips_pack_<fmt> (vbx_clips_pack.hpp, k_clips.hip).  Nothing here is a kernel of its own: a byte is
// decoded in registers by the readers' arithmetic (vbx_reader.hpp: byte_value, read_one<FMT>, lds_one<FMT>, read_group_wide<FMT>) on
// its way into the typed plane -- G.711 to the int16 the PCM16 kernels read, unsigned 8-bit PCM to a double -- so an 8-bit source
// costs the same launches as a 16-bit one and no decoded copy exists besides the plane.  The per-channel readers' 8-bit
// instantiations (unpack_<fmt>, unpack_all_<fmt>, session_ingest_<fmt>) are in k_reader.hip and k_session.hip beside the others.
#include "vbx_device.hpp"
#include "vbx_kernels.hpp"
#include "vbx_reader.hpp"
#include "vbx_session_ingest_all.hpp"
#include "vbx_clips_pack.hpp"

namespace vbx {

void launch_session_ingest_all8(hipStream_t s, int format, const void *old, size_t old_ld, size_t drop, size_t keep, const void *raw,
                                size_t n_new, size_t channels, const unpack_sel_t &sel, size_t n_sel, void *out, size_t out_ld) {
    if (keep + n_new == 0 || n_sel == 0) return;
    switch (format) {
        case UNPACK_U8: launch_ingest_all_as<UNPACK_U8>(s, old, old_ld, drop, keep, raw, n_new, channels, sel, n_sel, out, out_ld); break;
        case UNPACK_ULAW: launch_ingest_all_as<UNPACK_ULAW>(s, old, old_ld, drop, keep, raw, n_new, channels, sel, n_sel, out, out_ld); break;
        case UNPACK_ALAW: launch_ingest_all_as<UNPACK_ALAW>(s, old, old_ld, drop, keep, raw, n_new, channels, sel, n_sel, out, out_ld); break;
    }
}

void launch_clips_pack8(hipStream_t s, int format, const clip_entry_t *tab, size_t n, size_t total, void *plane) {
    if (n == 0 || total == 0) return;
    switch (format) {
        case UNPACK_U8: launch_pack_as<UNPACK_U8>(s, tab, n, total, plane); break;
        case UNPACK_ULAW: launch_pack_as<UNPACK_ULAW>(s, tab, n, total, plane); break;
        case UNPACK_ALAW: launch_pack_as<UNPACK_ALAW>(s, tab, n, total, plane); break;
    }
}

}  // namespace vbx
