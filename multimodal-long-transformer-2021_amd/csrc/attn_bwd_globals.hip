// The per-example-global-token (MMT_FLAG_EXAMPLE_GLOBALS) instantiations of the general backward kernels, as a translation
// unit of their own: attn_bwd.hip's kernel templates with ORG = true and GLB = true, and launch_attn_bwd_globals.  Built
// beside attn_bwd.o, as attn_bwd_origin.o is.
#define MMT_GLOBALS_TU 1
#include "attn_bwd.hip"
