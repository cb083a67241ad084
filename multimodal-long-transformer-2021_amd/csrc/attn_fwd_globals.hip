// The per-example-global-token (MMT_FLAG_EXAMPLE_GLOBALS) instantiations of the general forward kernel, as a translation
// unit of their own: attn_fwd.hip's kernel template with ORG = true and GLB = true, and launch_attn_fwd_globals.  Built
// beside attn_fwd.o, as attn_fwd_origin.o is.
#define MMT_GLOBALS_TU 1
#include "attn_fwd.hip"
