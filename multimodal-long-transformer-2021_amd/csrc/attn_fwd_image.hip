// The MMT_IDS_2D_IMAGE (2-D ids with the image at ids_go) instantiations of the general forward kernel, as a translation
// unit of their own: attn_fwd.hip's kernel template with rel_id reading the origin, and launch_attn_fwd_image.  Built beside
// attn_fwd.o like attn_fwd_origin.o; the instantiations of the other two units never read the origin.
#define MMT_IMAGE_TU 1
#include "attn_fwd.hip"
