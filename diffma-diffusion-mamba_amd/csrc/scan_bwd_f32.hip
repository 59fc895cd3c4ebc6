// scan_bwd: f32 I/O instantiations (split per dtype so the library builds in parallel)
#include "scan_bwd_chunked.h"
namespace dm {
int scan_bwd_f32(const dm_scan_bwd_args& a, const dm_scan_bwd_args* second, hipStream_t st) { return bwd_dispatch<float>(a, second, st); }
bool scan_bwd_takes_two(const dm_scan_bwd_args& a) { return bwd_goes_chunked(a) > 0; }
}  // namespace dm

extern "C" int dm_scan_bwd_group_channels(int dstate) {
    using namespace dm;
    switch (dstate) {
        case 16: return (WAVE / bwd_split<16>::value) * BWD_WAVES;
#ifndef DM_FAST_BUILD
        case 8: return (WAVE / bwd_split<8>::value) * BWD_WAVES;
        case 32: return (WAVE / bwd_split<32>::value) * BWD_WAVES;
        case 64: return (WAVE / bwd_split<64>::value) * BWD_WAVES;
        case 128: return (WAVE / bwd_split<128>::value) * BWD_WAVES;
#endif
        default: return -1;
    }
}

// channels per dB/dC partial row for THIS launch: 64 when the chunk-parallel kernel (scan_bwd_chunked.h) will take it,
// dm_scan_bwd_group_channels(dstate) otherwise.  The host sizes dBC_partial [nseq][seqlen][ceil(dim/GC)][2*dstate] with it.
extern "C" int dm_scan_bwd_launch_group_channels(int nseq, int dim, int seqlen, int dstate, int flags) {
    if (dm::bwd_chunked_lc(nseq, dim, seqlen, dstate, flags) > 0) return dm::WAVE;
    return dm_scan_bwd_group_channels(dstate);
}

// tokens per segment of the chunk-parallel backward (scan_bwd_chunked.h) when a launch of this size -- with arguments the family
// accepts -- takes it; 0 when it takes the sequential kernel.  The backward twin of dm_scan_fwd_launch_segment.
extern "C" int dm_scan_bwd_launch_segment(int nseq, int dim, int seqlen, int dstate, int flags) {
    return dm::bwd_chunked_segment(nseq, dim, seqlen, dstate, flags);
}
