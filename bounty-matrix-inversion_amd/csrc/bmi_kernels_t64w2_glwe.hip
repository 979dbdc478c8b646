// The entries of bmi_kernels_t64w2.hip that return the accumulator instead of the extracted sample (k_blind_rotate_*_glwe and their
// launchers launch_blind_rotate_*_glwe): the same kernel text, compiled a second time with the other epilogue - see BMI_ROT_ENTRY
// in bmi_internal.hpp.  A translation unit of its own, so that the object code of the existing entries stays what it was.
#define BMI_ROT_GLWE 1
#include "bmi_kernels_t64w2.hip"
