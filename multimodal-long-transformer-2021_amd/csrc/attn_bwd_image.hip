// The MMT_IDS_2D_IMAGE (2-D ids with the image at ids_go) instantiations of the general backward kernels, as a translation
// unit of their own: attn_bwd.hip's kernel templates with rel_id reading the origin, and launch_attn_bwd_image (see
// attn_fwd_image.hip).
#define MMT_IMAGE_TU 1
#include "attn_bwd.hip"
