// The 6-bit shadow of a Float32 corpus in the 5+1 LAYOUT (shadow_5p1.h; api.hip: the one-query shadow stream where the layout
// is no larger than the 6-bit one): K1's 6-bit unit reading five bits of every row and the sixth only of the rows whose best
// possible key still reaches the margin of the search's k-th best (scan_stream.inc, S51).  The keys of the rows that reach a
// list are the 6-bit unit's, bit for bit.
#define MVF_SCAN_DT 2
#define MVF_SCAN_XS 3
#include "scan_stream.inc"
