// The own-nodes run forms of the all-feature kernel (simon_wide.hip: wide_kernel<T, false, 3> without and <T, false, 4> with Open-Local:
// segmented and node-subset batches, where a scenario holds the pool nodes its rank row ranks below N) as a translation unit of their
// own: build() runs one hipcc process per unit, and the instantiations of the prefix forms keep their names and their code.
#define SIMON_WIDE_OWN_TU 1
#include "simon_wide.hip"
