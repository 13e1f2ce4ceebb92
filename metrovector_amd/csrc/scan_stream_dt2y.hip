// The 6-BIT SHADOW of a Float32 corpus (shadow_6b.hip; api.hip: ONE query, scan path 0 from kStream6MinBytes on, scan path 7):
// K1 with one lane per row over 64-row tiles, the query at sixteen bits in two int8 planes, exact i32 dot products per plane
// and the int8 unit's float keys.
#define MVF_SCAN_DT 2
#define MVF_SCAN_XS 2
#include "scan_stream.inc"
