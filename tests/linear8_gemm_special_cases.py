"""antq_linear8_gemm's entry in the special-value cases of linear_special_cases.py: the description of the entry point is
registered here, beside the five that module holds, and its builders and its order-independent expectation then make the cases
(non-finite weights, inputs and biases, the padded tail of K, the edges of the one rounding).  linear_special_cases.SETS is
computed when that module is imported and stays as it is: the tests parametrised over it do not change.

The tiled kernel with byte codes (csrc/antq_k_linear_gemm.h with Lin8Codec): steps of 128 elements on both code paths; a lane
past the end of K repeats the row's last load unit -- 16 bytes on the 16-byte path (at K % 32 == 16 the last lane group's own
second load), 8 bytes on the narrow one; K = 256 has no tail."""
import linear_special_cases as sc

ENTRY = "linear8_gemm"
sc.ENTRIES[ENTRY] = dict(width=8, narrow=(8, 136, 264), wide=(16, 144, 272, 256), unit={True: 16, False: 8}, step={True: 128, False: 128}, off=8,
                         Ms=(1, 65, 129, 257), NK=sc.ENTRIES["linear4_gemm"]["NK"], knob=23, edges=(63, 64, 127, 128), pads=True,
                         dtypes=("bfloat16", "float16"))
SETS = tuple((ENTRY, d) for d in sc.ENTRIES[ENTRY]["dtypes"])
