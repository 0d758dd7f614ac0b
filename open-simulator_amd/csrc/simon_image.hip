// simon_image.hip -- table_image_kernel (simon_table.hip): the initial score table of a batch's largest scenario, written once per run, from which
// the one-level kernels of simon_table.hip copy their prologue.  A translation unit of its own: build() runs one hipcc process per unit.
#define SIMON_IMAGE_TU 1
#include "simon_table.hip"
