// The block formats of the quantised frozen base (include/dta.h "Quantised frozen base"): constants shared by host and
// device code.  The NF4 code book stands here ONCE as fp32 literals; quant.py holds the one Python copy, and tests/test_quant_host.py
// compares the two bit for bit and recomputes the construction (normal quantiles, normalised) in float64.
#ifndef DTA_QUANT_TABLES_H
#define DTA_QUANT_TABLES_H

#define DTA_NF4_BLOCK 64
#define DTA_FP8_BLOCK 128
#define DTA_FP8_MAX 448.0f       /* largest finite OCP e4m3 value */

// DTA_NF4_CODEBOOK_BEGIN
#define DTA_NF4_CODEBOOK \
  -1.0f, -0.6961928009986877f, -0.5250730514526367f, -0.39491748809814453f, -0.28444138169288635f, -0.18477343022823334f, \
  -0.09105003625154495f, 0.0f, 0.07958029955625534f, 0.16093020141124725f, 0.24611230194568634f, 0.33791524171829224f, \
  0.44070982933044434f, 0.5626170039176941f, 0.7229568362236023f, 1.0f
// DTA_NF4_CODEBOOK_END

// mid_i = (c_i + c_{i+1}) / 2, formed in float64 (the sum of two floats and its half are exact there) and rounded once to fp32
#define DTA_NF4_MID(c, i) ((float)(((double)(c)[i] + (double)(c)[(i) + 1]) / 2.0))

#endif
