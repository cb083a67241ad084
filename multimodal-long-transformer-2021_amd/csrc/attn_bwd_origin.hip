// The per-example-origin (MMT_FLAG_EXAMPLE_STARTS) instantiations of the general backward kernels, as a translation unit
// of their own: attn_bwd.hip's kernel templates with ORG = true, and launch_attn_bwd_origin (see attn_fwd_origin.hip).
#define MMT_ORIGIN_TU 1
#include "attn_bwd.hip"
