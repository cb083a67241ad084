// The per-example-origin (MMT_FLAG_EXAMPLE_STARTS) instantiations of the general forward kernel, as a translation unit
// of their own: attn_fwd.hip's kernel template with ORG = true, and launch_attn_fwd_origin.  Built beside attn_fwd.o, so
// that the library's build time grows by a parallel job and not by the length of its longest one.
#define MMT_ORIGIN_TU 1
#include "attn_fwd.hip"
