"""Every kernel form behind the operator-level convolution ABI against fp64, form by form.  `pytest -m gpu`.

E-RAFT (inference under autograd, training) and EEMFlow+ training go through eemop_conv2d_fwd / _bwd_data / _bwd_weight / _bwd_weight_cat,
whose dispatch chooses between 193 named kernel forms.  Every case here pins the dispatch switches, makes ONE ABI call,
asserts by `eemop_last_conv_form` that the intended instantiation ran, and holds the result to the limits of that form's family
(oracle/fp64_bounds.py: FORM_FAMILY -> LIMITS; no limit is fitted to these kernels) in units of fp32 rounding of the output's own sum,
z = (got - ref) / (2^-24 sum |terms|), naming the worst element's tile on failure.  tests/test_fp64_bounds_ops.py shows on the CPU that
these checks reject a dropped bf16 piece, a dropped tap at a tile edge, a 3 u scale error, swapped segments, a missing image, a slice
one channel off, a missing parity class and `=` for `+=` - and pass torch's fp32 evaluation with room to spare.

Inputs are seeded; weights and biases have nn.Conv2d's default initialisation; upstream gradients are random-sign.  Shapes cut every
form's tiles on the right and at the bottom and use batch > 1 where the grid has a batch axis.  Every forward case writes into a channel
slice of a wider, sentinel-filled buffer, which must come back bitwise; the epilogue (none / ReLU / LeakyReLU) and out_scale rotate over
the cases.  Weight gradients accumulate with fp32 atomics: every case runs four times on seeded prefills of dw and db, `got - prefill` is
held to the limits each time, and one run passes db = NULL.  `test_every_form_in_the_table_ran` compares the names seen with the table.

LEFT OUT, and why:
  * sigmoid and tanh epilogues: the accuracy of a transcendental is a different contract from a sum's rounding; the E-RAFT goldens
    cover them.
  * the fused epilogues GEPI_MUL / GEPI_GRU / GEPI_ZR / GEPI_ADD_RELU / GEPI_SUM2 and `pre`: this ABI does not reach them, only
    eraft_forward does.
  * conv_wnc.hip: this ABI does not reach it; the EEMFlow decoders' use of it is checked under EEM_DEC_WNC=1.
  * conv_stem7.hip: it reports "stem7_c<cin>", but only eraft_forward hands gconv_launch its packing - this ABI serves the 7x7 stride-2
    stems on the taps kernel (cases below); the E-RAFT goldens cover stem7.

MEASURED worst statistics per form (one AMD Instinct MI355X, gfx950, 256 CUs; over all cases and, for the weight gradients, all four
runs; the slope over the tensors of at least 256 values).  A record: these numbers set no limit.  The closest to a limit is gconvb's
slope at 384 input channels, 2.3 - 2.4 u of bx3's 2.4 u: the three products of the smallest pieces that a bf16-piece multiply leaves out
have the sign of the product they belong to (the pieces are cut by truncation), a scale error of up to 2 u by construction.
  form                                     family          max|z|    rms   |mean|  |slope| u  checks
  dgrad_s2w_128_1x1                        dgrad_s2          4.70  0.218   0.0002    0.004       1
  dgrad_s2w_128_3x3                        dgrad_s2          5.30  0.434   0.0001    0.002       1
  dgrad_s2w_96_1x1                         dgrad_s2          4.18  0.218   0.0001    0.002       1
  dgrad_s2w_96_3x3                         dgrad_s2          5.10  0.435   0.0003    0.014       1
  dgrad_t2_generic_1x1                     dgrad_gconv       4.17  0.218   0.0003    0.001       1
  dgrad_t2_generic_1x1_b1                  dgrad_gconv       3.31  0.440   0.0004    0.001       1
  dgrad_t2_generic_1x1_b4                  dgrad_gconv       4.46  0.439   0.0005    0.006       1
  dgrad_t2_generic_2x1                     dgrad_gconv       5.23  0.438   0.0001    0.006       3
  dgrad_t2_generic_2x2                     dgrad_gconv       4.79  0.217   0.0001    0.002       1
  dgrad_t2_generic_2x2_b1                  dgrad_gconv       3.52  0.441   0.0001    0.001       1
  dgrad_t2_generic_2x2_b4                  dgrad_gconv       4.85  0.441   0.0001    0.002       1
  dgrad_t2_generic_splitk16                dgrad_gconv       1.30  0.191   0.0003        -       2
  dgrad_t2_generic_splitk4                 dgrad_gconv       2.89  0.315   0.0005    0.006       3
  dgrad_t2_generic_splitk8                 dgrad_gconv       1.61  0.229   0.0002        -       1
  fewout_k16_c2                            direct            0.48  0.084   0.0068    0.463       1
  fewout_k16_c8                            direct            0.71  0.135   0.0018    0.140       3
  fewout_k8_c2                             direct            0.77  0.182   0.0115    0.031       2
  fewout_k8_c4                             direct            1.08  0.167   0.0038    0.150       2
  fewout_k8_c8                             direct            1.21  0.185   0.0037    0.009       3
  fewout_wide2                             direct            0.45  0.096   0.0019    0.151       2
  gconv16_1x1_s2                           direct            4.54  0.309   0.0000    0.006       1
  gconv16_1x1_th2_wm2_kg1                  direct            3.67  0.301   0.0004    0.023       1
  gconv16_1x1_th2_wm2_kg2                  direct            1.78  0.223   0.0071    0.087       1
  gconv16_1x1_th2_wm4_kg1                  direct            3.51  0.438   0.0039    0.010       1
  gconv16_1x1_th2_wm4_kg2                  direct            2.75  0.321   0.0012    0.012       2
  gconv16_1x1_th3_wm4_kg1                  direct            3.66  0.303   0.0023    0.024       1
  gconv16_1x1_th3_wm4_kg2                  direct            2.50  0.324   0.0034    0.001       1
  gconv16_1x1_th4_wm1_kg1                  direct            2.61  0.303   0.0073    0.110       1
  gconv16_1x1_th4_wm1_kg2                  direct            1.76  0.231   0.0012    0.006       1
  gconv16_1x1_th4_wm2_kg1                  direct            4.83  0.433   0.0004    0.001       1
  gconv16_1x1_th4_wm4_kg1                  direct            4.16  0.305   0.0030    0.022       1
  gconv16_1x1_th4_wm4_kg2                  direct            2.63  0.222   0.0000    0.000       1
  gconv16_1x1_th5_wm4_kg1                  direct            5.30  0.434   0.0037    0.001       1
  gconv16_1x1_th5_wm4_kg2                  direct            2.64  0.230   0.0010    0.021       1
  gconv16_1x1_th6_wm4_kg1                  direct            4.57  0.306   0.0042    0.049       1
  gconv16_1x1_th6_wm4_kg2                  direct            2.96  0.325   0.0017    0.001       1
  gconv16_1x5_th2_wm2_kg1                  direct            3.24  0.315   0.0054    0.228       1
  gconv16_1x5_th2_wm2_kg2                  direct            1.57  0.221   0.0018    0.008       1
  gconv16_1x5_th2_wm4_kg1                  direct            4.09  0.433   0.0017    0.037       1
  gconv16_1x5_th2_wm4_kg2                  direct            3.00  0.309   0.0006    0.019       3
  gconv16_1x5_th3_wm4_kg1                  direct            4.02  0.308   0.0014    0.022       1
  gconv16_1x5_th3_wm4_kg2                  direct            2.60  0.311   0.0010    0.004       1
  gconv16_1x5_th4_wm1_kg1                  direct            2.92  0.312   0.0062    0.055       1
  gconv16_1x5_th4_wm1_kg2                  direct            1.43  0.217   0.0039    0.135       1
  gconv16_1x5_th4_wm2_kg1                  direct            5.31  0.437   0.0019    0.001       1
  gconv16_1x5_th4_wm4_kg1                  direct            3.98  0.307   0.0012    0.020       1
  gconv16_1x5_th4_wm4_kg2                  direct            2.25  0.219   0.0003    0.009       1
  gconv16_1x5_th5_wm4_kg1                  direct            4.95  0.435   0.0010    0.009       1
  gconv16_1x5_th5_wm4_kg2                  direct            2.65  0.223   0.0008    0.025       1
  gconv16_1x5_th6_wm4_kg1                  direct            4.32  0.308   0.0011    0.030       1
  gconv16_1x5_th6_wm4_kg2                  direct            2.84  0.311   0.0008    0.003       1
  gconv16_3x3_s2                           direct            5.64  0.307   0.0000    0.004       1
  gconv16_3x3_th2_wm2_kg1                  direct            2.60  0.311   0.0026    0.083       1
  gconv16_3x3_th2_wm2_kg2                  direct            1.80  0.222   0.0011    0.031       1
  gconv16_3x3_th2_wm4_kg1                  direct            3.46  0.438   0.0037    0.097       1
  gconv16_3x3_th2_wm4_kg2                  direct            2.69  0.316   0.0010    0.160       4
  gconv16_3x3_th3_wm4_kg1                  direct            3.76  0.309   0.0006    0.008       1
  gconv16_3x3_th3_wm4_kg2                  direct            3.14  0.311   0.0016    0.024       3
  gconv16_3x3_th4_wm1_kg1                  direct            4.31  0.317   0.0067    0.181       1
  gconv16_3x3_th4_wm1_kg2                  direct            1.86  0.226   0.0071    0.181       1
  gconv16_3x3_th4_wm2_kg1                  direct            6.24  0.433   0.0006    0.006       1
  gconv16_3x3_th4_wm4_kg1                  direct            4.43  0.306   0.0004    0.025       1
  gconv16_3x3_th4_wm4_kg2                  direct            2.38  0.219   0.0003    0.002       1
  gconv16_3x3_th5_wm4_kg1                  direct            4.88  0.435   0.0033    0.015       1
  gconv16_3x3_th5_wm4_kg2                  direct            3.01  0.222   0.0002    0.012       1
  gconv16_3x3_th6_wm4_kg1                  direct            4.42  0.311   0.0003    0.004       1
  gconv16_3x3_th6_wm4_kg2                  direct            3.05  0.308   0.0000    0.006       1
  gconv16_5x1_th2_wm2_kg1                  direct            3.64  0.311   0.0025    0.027       1
  gconv16_5x1_th2_wm2_kg2                  direct            1.70  0.220   0.0044    0.162       1
  gconv16_5x1_th2_wm4_kg1                  direct            3.14  0.434   0.0022    0.070       1
  gconv16_5x1_th2_wm4_kg2                  direct            2.75  0.309   0.0017    0.081       3
  gconv16_5x1_th3_wm4_kg1                  direct            4.96  0.308   0.0011    0.036       1
  gconv16_5x1_th3_wm4_kg2                  direct            2.41  0.310   0.0006    0.016       1
  gconv16_5x1_th4_wm1_kg1                  direct            3.14  0.304   0.0008    0.049       1
  gconv16_5x1_th4_wm1_kg2                  direct            1.62  0.218   0.0002    0.042       1
  gconv16_5x1_th4_wm2_kg1                  direct            6.18  0.432   0.0011    0.002       1
  gconv16_5x1_th4_wm4_kg1                  direct            3.71  0.309   0.0001    0.022       1
  gconv16_5x1_th4_wm4_kg2                  direct            2.32  0.219   0.0002    0.006       1
  gconv16_5x1_th5_wm4_kg1                  direct            4.18  0.433   0.0005    0.004       1
  gconv16_5x1_th5_wm4_kg2                  direct            3.32  0.223   0.0005    0.007       1
  gconv16_5x1_th6_wm4_kg1                  direct            4.45  0.307   0.0006    0.009       1
  gconv16_5x1_th6_wm4_kg2                  direct            2.44  0.311   0.0002    0.002       1
  gconvb_1x1_th2                           bx3               2.81  0.311   0.0498    0.799       2
  gconvb_1x1_th4                           bx3               2.22  0.236   0.0862    0.845       1
  gconvb_1x1_th6                           bx3               2.31  0.226   0.0729    0.759       1
  gconvb_1x1_th8                           bx3               2.83  0.316   0.0278    0.704       1
  gconvb_1x5_th2                           bx3               3.55  0.365   0.0373    0.763       3
  gconvb_1x5_th4                           bx3               4.32  0.354   0.0349    2.369       2
  gconvb_1x5_th6                           bx3               4.41  0.253   0.0434    0.872       1
  gconvb_1x5_th8                           bx3               4.13  0.254   0.0402    0.875       1
  gconvb_3x3_th2                           bx3               3.32  0.262   0.0332    1.519       2
  gconvb_3x3_th4                           bx3               3.27  0.257   0.0313    0.875       1
  gconvb_3x3_th6                           bx3               3.93  0.357   0.0187    0.639       1
  gconvb_3x3_th8                           bx3               4.63  0.254   0.0310    0.860       1
  gconvb_5x1_th2                           bx3               3.86  0.359   0.0335    1.050       2
  gconvb_5x1_th4                           bx3               4.13  0.269   0.0422    2.321       2
  gconvb_5x1_th6                           bx3               4.04  0.254   0.0388    0.860       1
  gconvb_5x1_th8                           bx3               4.04  0.353   0.0165    0.732       1
  generic_1x1                              direct            4.14  0.442   0.0036    0.038       3
  generic_1x1_b1                           direct            2.07  0.305   0.0039    0.008       1
  generic_1x1_b4                           direct            3.91  0.304   0.0023    0.037       1
  generic_2x1                              direct            5.06  0.308   0.0000    0.000       1
  generic_2x2                              direct            5.20  0.434   0.0018    0.000       1
  generic_2x2_b1                           direct            3.49  0.327   0.0011    0.000       1
  generic_2x2_b4                           direct            5.25  0.435   0.0014    0.001       1
  generic_splitk16                         direct            0.59  0.121   0.0008    0.024       2
  generic_splitk4                          direct            1.81  0.227   0.0012    0.016       5
  generic_splitk8                          direct            1.03  0.166   0.0007    0.093       4
  taps_3x3                                 direct            4.49  0.437   0.0040    0.052       3
  taps_7x7                                 direct            4.52  0.435   0.0033    0.046       6
  wgrad_enc_bx3_tw16_c32_s1                wgrad_bx3         0.63  0.088   0.0308    0.747       7
  wgrad_enc_bx3_tw16_c32_s2                wgrad_bx3         0.56  0.084   0.0302    0.648       7
  wgrad_enc_bx3_tw16_c64_s1                wgrad_bx3         0.65  0.087   0.0312    0.690      14
  wgrad_enc_bx3_tw16_c64_s2                wgrad_bx3         0.62  0.087   0.0295    0.687       7
  wgrad_enc_bx3_tw32_c32_s1                wgrad_bx3         0.65  0.100   0.0274    0.707       7
  wgrad_enc_bx3_tw32_c32_s2                wgrad_bx3         0.61  0.081   0.0304    0.642       7
  wgrad_enc_bx3_tw32_c64_s1                wgrad_bx3         0.57  0.080   0.0276    0.691       7
  wgrad_enc_bx3_tw32_c64_s2                wgrad_bx3         0.65  0.080   0.0273    0.700       7
  wgrad_enc_fp32_tw16_c16_s1               wgrad_fp32        0.62  0.089   0.0262    0.056       7
  wgrad_enc_fp32_tw16_c16_s2               wgrad_fp32        0.43  0.086   0.0127    0.209       7
  wgrad_enc_fp32_tw16_c32_s1               wgrad_fp32        0.58  0.089   0.0109    0.039       7
  wgrad_enc_fp32_tw16_c32_s2               wgrad_fp32        0.71  0.089   0.0026    0.022       7
  wgrad_enc_fp32_tw16_c64_s1               wgrad_fp32        0.68  0.088   0.0097    0.046      14
  wgrad_enc_fp32_tw16_c64_s2               wgrad_fp32        0.65  0.088   0.0058    0.022       7
  wgrad_enc_fp32_tw32_c16_s1               wgrad_fp32        0.53  0.087   0.0194    0.167       7
  wgrad_enc_fp32_tw32_c16_s2               wgrad_fp32        0.47  0.085   0.0088    0.091       7
  wgrad_enc_fp32_tw32_c32_s1               wgrad_fp32        0.64  0.082   0.0140    0.050       7
  wgrad_enc_fp32_tw32_c32_s2               wgrad_fp32        0.56  0.082   0.0255    0.058       7
  wgrad_enc_fp32_tw32_c5_c16_s2            wgrad_fp32        0.66  0.173   0.0229    0.101       7
  wgrad_enc_fp32_tw32_c64_s1               wgrad_fp32        0.56  0.083   0.0101    0.040       7
  wgrad_enc_fp32_tw32_c64_s2               wgrad_fp32        0.59  0.081   0.0149    0.022       7
  wgrad_few_c2                             wgrad_batched     1.05  0.199   0.0925    0.035      21
  wgrad_few_c4                             wgrad_batched     1.05  0.198   0.0801    0.024      14
  wgrad_few_c8                             wgrad_batched     1.08  0.182   0.0504    0.007      14
  wgrad_generic_1x1_s1                     wgrad_batched     1.11  0.223   0.0030    0.004       1
  wgrad_generic_1x1_s1_bias                wgrad_batched     1.42  0.224   0.0124    0.014       6
  wgrad_generic_1x1_s2                     wgrad_batched     1.34  0.213   0.0010    0.001       1
  wgrad_generic_1x1_s2_bias                wgrad_batched     1.46  0.214   0.0043    0.022       6
  wgrad_generic_1x5_s1                     wgrad_batched     1.22  0.225   0.0002    0.003       1
  wgrad_generic_1x5_s1_bias                wgrad_batched     1.22  0.227   0.0158    0.007       6
  wgrad_generic_3x3_s1                     wgrad_batched     1.61  0.232   0.0011    0.013       4
  wgrad_generic_3x3_s1_bias                wgrad_batched     1.76  0.232   0.0285    0.012      18
  wgrad_generic_3x3_s1_bias + wgrad_generic_3x3_s1 wgrad_batched     1.47  0.231   0.0181    0.013       6
  wgrad_generic_3x3_s2                     wgrad_batched     1.41  0.218   0.0002    0.023       1
  wgrad_generic_3x3_s2_bias                wgrad_batched     1.41  0.219   0.0236    0.019       6
  wgrad_generic_5x1_s1                     wgrad_batched     1.25  0.231   0.0017    0.045       1
  wgrad_generic_5x1_s1_bias                wgrad_batched     1.48  0.234   0.0161    0.038       6
  wgrad_generic_7x7_s1                     wgrad_batched     1.56  0.282   0.0034    0.019       1
  wgrad_generic_7x7_s1_bias                wgrad_batched     1.61  0.284   0.0050    0.022       6
  wgrad_generic_7x7_s2                     wgrad_batched     1.26  0.258   0.0009    0.038       1
  wgrad_generic_7x7_s2_bias                wgrad_batched     1.40  0.259   0.0097    0.038       6
  wgrad_ring_1616                          wgrad_ring        0.82  0.112   0.0174    0.196       7
  wgrad_ring_1616_cat2                     wgrad_ring        0.88  0.126   0.0421    0.132       7
  wgrad_ring_1616_cat3                     wgrad_ring        0.86  0.125   0.0251    0.086       7
  wgrad_ring_3232                          wgrad_ring        0.85  0.114   0.0132    0.046       7
  wgrad_ring_3232_cat2                     wgrad_ring        1.02  0.128   0.0150    0.054       7
  wgrad_ring_3232_cat3                     wgrad_ring        1.08  0.131   0.0077    0.033       7
  wgrad_ring_6464                          wgrad_ring        1.21  0.123   0.0254    0.041      14
  wgrad_ring_6464_cat2                     wgrad_ring        1.24  0.138   0.0237    0.015      14
  wgrad_ring_6464_cat3                     wgrad_ring        1.41  0.139   0.0172    0.014      14
  wgrad_ring_s2_3216                       wgrad_ring        0.74  0.088   0.0112    0.183       7
  wgrad_ring_s2_3216_cat2                  wgrad_ring        0.94  0.125   0.0059    0.085       7
  wgrad_ring_s2_3216_cat3                  wgrad_ring        1.11  0.130   0.0120    0.111       7
  wgrad_ring_s2_6432                       wgrad_ring        0.73  0.097   0.0063    0.060       7
  wgrad_ring_s2_6432_cat2                  wgrad_ring        0.99  0.129   0.0110    0.042       7
  wgrad_ring_s2_6432_cat3                  wgrad_ring        1.06  0.131   0.0080    0.044       7
  wgrad_ring_s2_6464                       wgrad_ring        0.87  0.104   0.0073    0.039      14
  wgrad_ring_s2_6464_cat2                  wgrad_ring        1.11  0.137   0.0229    0.044       7
  wgrad_ring_s2_6464_cat3                  wgrad_ring        0.86  0.130   0.0113    0.010       7
  wgrad_ring_wide_1x5                      wgrad_ring        0.97  0.123   0.0168    0.051       7
  wgrad_ring_wide_1x5_cat2                 wgrad_ring        1.02  0.139   0.0123    0.029      14
  wgrad_ring_wide_1x5_cat3                 wgrad_ring        1.55  0.139   0.0264    0.037      14
  wgrad_ring_wide_5x1_6432                 wgrad_ring        0.62  0.084   0.0057    0.051       7
  wgrad_ring_wide_5x1_6432_cat2            wgrad_ring        0.71  0.095   0.0043    0.029       7
  wgrad_ring_wide_5x1_6432_cat3            wgrad_ring        0.54  0.094   0.0124    0.024       7
  wgrad_ring_wide_5x1_6464                 wgrad_ring        1.05  0.123   0.0300    0.018       7
  wgrad_ring_wide_5x1_6464_cat2            wgrad_ring        1.31  0.138   0.0140    0.027      14
  wgrad_ring_wide_5x1_6464_cat3            wgrad_ring        1.44  0.138   0.0096    0.021      14
  wgrad_wide_bx3_tw16_1x1                  wgrad_bx3         0.59  0.084   0.0297    0.718       7
  wgrad_wide_bx3_tw16_1x5                  wgrad_bx3         0.74  0.086   0.0303    0.708      21
  wgrad_wide_bx3_tw16_3x3                  wgrad_bx3         0.78  0.087   0.0306    0.736      14
  wgrad_wide_bx3_tw16_5x1                  wgrad_bx3         0.66  0.087   0.0301    0.734       7
  wgrad_wide_bx3_tw32_1x1                  wgrad_bx3         0.53  0.080   0.0284    0.729       7
  wgrad_wide_bx3_tw32_1x5                  wgrad_bx3         0.61  0.079   0.0284    0.656       7
  wgrad_wide_bx3_tw32_3x3                  wgrad_bx3         0.62  0.081   0.0283    0.682       7
  wgrad_wide_bx3_tw32_5x1                  wgrad_bx3         0.73  0.081   0.0281    0.718       7
  wgrad_wide_fp32_tw16_1x1                 wgrad_fp32        0.49  0.087   0.0027    0.093       7
  wgrad_wide_fp32_tw16_1x5                 wgrad_fp32        0.65  0.089   0.0113    0.033       7
  wgrad_wide_fp32_tw16_3x3                 wgrad_fp32        0.68  0.088   0.0087    0.013       7
  wgrad_wide_fp32_tw16_5x1                 wgrad_fp32        0.70  0.090   0.0038    0.024       7
  wgrad_wide_fp32_tw32_1x1                 wgrad_fp32        0.60  0.082   0.0054    0.067       7
  wgrad_wide_fp32_tw32_1x5                 wgrad_fp32        0.69  0.080   0.0063    0.066       7
  wgrad_wide_fp32_tw32_3x3                 wgrad_fp32        0.60  0.082   0.0092    0.023       7
  wgrad_wide_fp32_tw32_5x1                 wgrad_fp32        0.72  0.081   0.0052    0.043       7
  dgrad_t2_generic_splitk16                KAPPA_DEC      error / torch fp32 CPU's error: rms 0.39, max 0.25 (limit 6.4)       2
  dgrad_t2_generic_splitk8                 KAPPA_DEC      error / torch fp32 CPU's error: rms 0.52, max 0.32 (limit 6.4)       1
"""
import ctypes
import zlib

import pytest
import torch

from eemflow_amd import _lib
from oracle import fp64_bounds as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345.678

# every switch the dispatch reads per call: unset unless a case sets it
SWITCHES = ("EEM_NO_FEWOUT", "EEM_FEWOUT_WIDE", "EEM_NO_TAPS_KERNEL", "EEM_NO_SPLITK", "EEM_NO_GCONV16", "EEM_NO_G16_S2", "EEM_NO_GCONVB",
            "EEM_GCONVB_1X1", "EEM_GCONVB_MINBLK", "EEM_NO_STEM7", "EEM_NO_DGRAD_S2W", "EEM_NO_WGRAD_RING", "EEM_WGRAD_RING",
            "EEM_WGRAD_RING_BLOCK", "EEM_WGRAD_RING_51", "EEM_NO_WGRAD_FEW", "EEM_NO_WGRAD_ENC", "EEM_NO_WGRAD_WIDE", "EEM_NO_WGRAD_BX3",
            "EEM_WGRAD_BURST")
SEEN = set()            # form names (the parts of '+'-joined ones) that ran
RAN = set()             # case ids that ran


def _pin(monkeypatch, env):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        assert name in SWITCHES, name
        monkeypatch.setenv(name, value)


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _sp():
    return _lib.current_stream_ptr(torch.device(DEV))


def _ptr(t):
    return t.data_ptr() if t is not None else None


def last_form():
    buf = ctypes.create_string_buffer(512)
    _lib.check(_lib.lib().eemop_last_conv_form(buf, len(buf)))
    return buf.value.decode()


def _tile(form):
    """(rows, columns) of a form's output tile, for the failure message."""
    f = form.split("+")[0]
    if f.startswith(("gconv16_", "gconvb_")):
        return (4 if f.endswith("_s2") else int(f.split("_th")[1].split("_")[0]), 16)
    if f.startswith("dgrad_s2w"):
        return (8, 16)
    return None


# ------------------------------------------------------------------------------------------- one ABI call each (GPU tensors in, CPU out)
def run_fwd(xs, w, b, stride, pad, act, out_scale, ctotal, coff):
    """eemop_conv2d_fwd into channels [coff, coff + cout) of a sentinel-filled [n][ctotal] buffer: (whole buffer, form)."""
    xs = [x.to(DEV).contiguous() for x in xs]
    w, b = w.to(DEV).contiguous(), (b.to(DEV).contiguous() if b is not None else None)
    n, _, hin, win = xs[0].shape
    cout, _, kh, kw = w.shape
    hout, wout = (hin + 2 * pad[0] - kh) // stride + 1, (win + 2 * pad[1] - kw) // stride + 1
    out = torch.full((n, ctotal, hout, wout), SENTINEL, device=DEV)
    px = [x.data_ptr() for x in xs] + [None] * (3 - len(xs))
    pc = [x.shape[1] for x in xs] + [0] * (3 - len(xs))
    _lib.check(_lib.lib().eemop_conv2d_fwd(px[0], pc[0], px[1], pc[1], px[2], pc[2], w.data_ptr(), _ptr(b), n, hin, win, cout, kh, kw, stride,
                                           pad[0], pad[1], act, float(out_scale), out.data_ptr(), ctotal, coff, _sp()))
    form = last_form()
    torch.cuda.synchronize()
    return out.cpu(), form


def run_dgrad(dy, w, in_hw, stride, pad, ci0, cic):
    dy, w = dy.to(DEV).contiguous(), w.to(DEV).contiguous()
    n = dy.shape[0]
    cout, cin, kh, kw = w.shape
    dx = torch.full((n, cic, *in_hw), SENTINEL, device=DEV)
    _lib.check(_lib.lib().eemop_conv2d_bwd_data(dy.data_ptr(), w.data_ptr(), n, in_hw[0], in_hw[1], cin, ci0, cic, cout, kh, kw, stride, pad[0],
                                                pad[1], dx.data_ptr(), _sp()))
    form = last_form()
    torch.cuda.synchronize()
    return dx.cpu(), form


def run_wgrad(xs, dy, wshape, stride, pad, ci0, pre_w, pre_b, cat):
    """dw / db += on the prefills (pre_b None: db = NULL): (dw, db or None, form).  cat: eemop_conv2d_bwd_weight_cat over the segments,
    else eemop_conv2d_bwd_weight on the one segment as the input-channel slice [ci0, ci0 + c) of wshape[1]."""
    xs = [x.to(DEV).contiguous() for x in xs]
    dy = dy.to(DEV).contiguous()
    n, _, hin, win = xs[0].shape
    cout, cin, kh, kw = wshape
    dw = pre_w.to(DEV).contiguous().clone()
    db = pre_b.to(DEV).contiguous().clone() if pre_b is not None else None
    L = _lib.lib()
    if cat:
        assert ci0 == 0 and sum(x.shape[1] for x in xs) == cin
        px = [x.data_ptr() for x in xs] + [None] * (3 - len(xs))
        pc = [x.shape[1] for x in xs] + [0] * (3 - len(xs))
        _lib.check(L.eemop_conv2d_bwd_weight_cat(px[0], pc[0], px[1], pc[1], px[2], pc[2], dy.data_ptr(), n, hin, win, cout, kh, kw, stride, pad[0],
                                                 pad[1], dw.data_ptr(), _ptr(db), _sp()))
    else:
        assert len(xs) == 1
        _lib.check(L.eemop_conv2d_bwd_weight(xs[0].data_ptr(), dy.data_ptr(), n, hin, win, cin, ci0, xs[0].shape[1], cout, kh, kw, stride, pad[0],
                                             pad[1], dw.data_ptr(), _ptr(db), _sp()))
    form = last_form()
    torch.cuda.synchronize()
    return dw.cpu(), (db.cpu() if db is not None else None), form


# ------------------------------------------------------------------------------------------------------------------------- cases
def _pad(k):
    return (k[0] // 2, k[1] // 2)


ACTS = (B.ACT_NONE, B.ACT_RELU, B.ACT_LEAKY)

# (form, input segments, cout, (kh, kw), stride, (ph, pw), n, h, w, switches)
FWD = [
    ('gconv16_1x1_th2_wm4_kg1', [48], 64, (1, 1), 1, (0, 0), 2, 9, 20, {}),
    ('gconv16_1x1_th2_wm4_kg2', [48, 32, 16], 64, (1, 1), 1, (0, 0), 2, 9, 20, {}),
    ('gconv16_1x1_th3_wm4_kg1', [32], 80, (1, 1), 1, (0, 0), 3, 43, 20, {}),
    ('gconv16_1x1_th3_wm4_kg2', [64], 80, (1, 1), 1, (0, 0), 3, 43, 20, {}),
    ('gconv16_1x1_th4_wm4_kg1', [48], 80, (1, 1), 1, (0, 0), 2, 97, 20, {}),
    ('gconv16_1x1_th4_wm4_kg2', [48, 32, 16], 80, (1, 1), 1, (0, 0), 2, 97, 20, {}),
    ('gconv16_1x1_th5_wm4_kg1', [32], 96, (1, 1), 1, (0, 0), 2, 129, 20, {}),
    ('gconv16_1x1_th5_wm4_kg2', [64], 96, (1, 1), 1, (0, 0), 2, 129, 20, {}),
    ('gconv16_1x1_th6_wm4_kg1', [32], 80, (1, 1), 1, (0, 0), 3, 106, 20, {}),
    ('gconv16_1x1_th6_wm4_kg2', [64], 80, (1, 1), 1, (0, 0), 3, 106, 20, {}),
    ('gconv16_1x1_th2_wm2_kg1', [48], 32, (1, 1), 1, (0, 0), 2, 9, 20, {}),
    ('gconv16_1x1_th2_wm2_kg2', [48, 32, 16], 32, (1, 1), 1, (0, 0), 2, 9, 20, {}),
    ('gconv16_1x1_th4_wm2_kg1', [32, 16], 32, (1, 1), 1, (0, 0), 3, 389, 100, {}),
    ('gconv16_1x1_th4_wm1_kg1', [32], 16, (1, 1), 1, (0, 0), 2, 9, 20, {}),
    ('gconv16_1x1_th4_wm1_kg2', [64], 16, (1, 1), 1, (0, 0), 2, 9, 20, {}),
    ('gconv16_3x3_th2_wm4_kg1', [48], 64, (3, 3), 1, (1, 1), 2, 9, 20, {}),
    ('gconv16_3x3_th2_wm4_kg2', [48, 32, 16], 64, (3, 3), 1, (1, 1), 2, 9, 20, {}),
    ('gconv16_3x3_th3_wm4_kg1', [32], 80, (3, 3), 1, (1, 1), 3, 43, 20, {}),
    ('gconv16_3x3_th3_wm4_kg2', [64], 80, (3, 3), 1, (1, 1), 3, 43, 20, {}),
    ('gconv16_3x3_th4_wm4_kg1', [48], 80, (3, 3), 1, (1, 1), 2, 97, 20, {}),
    ('gconv16_3x3_th4_wm4_kg2', [48, 32, 16], 80, (3, 3), 1, (1, 1), 2, 97, 20, {}),
    ('gconv16_3x3_th5_wm4_kg1', [32, 16], 80, (3, 3), 1, (1, 1), 2, 129, 20, {}),
    ('gconv16_3x3_th5_wm4_kg2', [80], 96, (3, 3), 1, (1, 1), 2, 129, 20, {}),
    ('gconv16_3x3_th6_wm4_kg1', [32], 80, (3, 3), 1, (1, 1), 3, 106, 20, {}),
    ('gconv16_3x3_th6_wm4_kg2', [64], 80, (3, 3), 1, (1, 1), 3, 106, 20, {}),
    ('gconv16_3x3_th2_wm2_kg1', [48], 32, (3, 3), 1, (1, 1), 2, 9, 20, {}),
    ('gconv16_3x3_th2_wm2_kg2', [48, 32, 16], 32, (3, 3), 1, (1, 1), 2, 9, 20, {}),
    ('gconv16_3x3_th4_wm2_kg1', [32, 16], 32, (3, 3), 1, (1, 1), 3, 389, 100, {}),
    ('gconv16_3x3_th4_wm1_kg1', [32], 16, (3, 3), 1, (1, 1), 2, 9, 20, {}),
    ('gconv16_3x3_th4_wm1_kg2', [64], 16, (3, 3), 1, (1, 1), 2, 9, 20, {}),
    ('gconv16_1x5_th2_wm4_kg1', [48], 64, (1, 5), 1, (0, 2), 2, 9, 20, {}),
    ('gconv16_1x5_th2_wm4_kg2', [48, 32, 16], 64, (1, 5), 1, (0, 2), 2, 9, 20, {}),
    ('gconv16_1x5_th3_wm4_kg1', [32], 80, (1, 5), 1, (0, 2), 3, 43, 20, {}),
    ('gconv16_1x5_th3_wm4_kg2', [64], 80, (1, 5), 1, (0, 2), 3, 43, 20, {}),
    ('gconv16_1x5_th4_wm4_kg1', [48], 80, (1, 5), 1, (0, 2), 2, 97, 20, {}),
    ('gconv16_1x5_th4_wm4_kg2', [48, 32, 16], 80, (1, 5), 1, (0, 2), 2, 97, 20, {}),
    ('gconv16_1x5_th5_wm4_kg1', [32, 16], 80, (1, 5), 1, (0, 2), 2, 129, 20, {}),
    ('gconv16_1x5_th5_wm4_kg2', [80], 96, (1, 5), 1, (0, 2), 2, 129, 20, {}),
    ('gconv16_1x5_th6_wm4_kg1', [32], 80, (1, 5), 1, (0, 2), 3, 106, 20, {}),
    ('gconv16_1x5_th6_wm4_kg2', [64], 80, (1, 5), 1, (0, 2), 3, 106, 20, {}),
    ('gconv16_1x5_th2_wm2_kg1', [48], 32, (1, 5), 1, (0, 2), 2, 9, 20, {}),
    ('gconv16_1x5_th2_wm2_kg2', [48, 32, 16], 32, (1, 5), 1, (0, 2), 2, 9, 20, {}),
    ('gconv16_1x5_th4_wm2_kg1', [32, 16], 32, (1, 5), 1, (0, 2), 3, 389, 100, {}),
    ('gconv16_1x5_th4_wm1_kg1', [32], 16, (1, 5), 1, (0, 2), 2, 9, 20, {}),
    ('gconv16_1x5_th4_wm1_kg2', [64], 16, (1, 5), 1, (0, 2), 2, 9, 20, {}),
    ('gconv16_5x1_th2_wm4_kg1', [48], 64, (5, 1), 1, (2, 0), 2, 9, 20, {}),
    ('gconv16_5x1_th2_wm4_kg2', [48, 32, 16], 64, (5, 1), 1, (2, 0), 2, 9, 20, {}),
    ('gconv16_5x1_th3_wm4_kg1', [32], 80, (5, 1), 1, (2, 0), 3, 43, 20, {}),
    ('gconv16_5x1_th3_wm4_kg2', [64], 80, (5, 1), 1, (2, 0), 3, 43, 20, {}),
    ('gconv16_5x1_th4_wm4_kg1', [48], 80, (5, 1), 1, (2, 0), 2, 97, 20, {}),
    ('gconv16_5x1_th4_wm4_kg2', [48, 32, 16], 80, (5, 1), 1, (2, 0), 2, 97, 20, {}),
    ('gconv16_5x1_th5_wm4_kg1', [32, 16], 80, (5, 1), 1, (2, 0), 2, 129, 20, {}),
    ('gconv16_5x1_th5_wm4_kg2', [80], 96, (5, 1), 1, (2, 0), 2, 129, 20, {}),
    ('gconv16_5x1_th6_wm4_kg1', [32], 80, (5, 1), 1, (2, 0), 3, 106, 20, {}),
    ('gconv16_5x1_th6_wm4_kg2', [64], 80, (5, 1), 1, (2, 0), 3, 106, 20, {}),
    ('gconv16_5x1_th2_wm2_kg1', [48], 32, (5, 1), 1, (2, 0), 2, 9, 20, {}),
    ('gconv16_5x1_th2_wm2_kg2', [48, 32, 16], 32, (5, 1), 1, (2, 0), 2, 9, 20, {}),
    ('gconv16_5x1_th4_wm2_kg1', [32, 16], 32, (5, 1), 1, (2, 0), 3, 389, 100, {}),
    ('gconv16_5x1_th4_wm1_kg1', [32], 16, (5, 1), 1, (2, 0), 2, 9, 20, {}),
    ('gconv16_5x1_th4_wm1_kg2', [64], 16, (5, 1), 1, (2, 0), 2, 9, 20, {}),
    ('gconvb_1x1_th2', [32], 96, (1, 1), 1, (0, 0), 1, 7, 20, {'EEM_GCONVB_1X1': '1', 'EEM_GCONVB_MINBLK': '1'}),
    ('gconvb_1x1_th4', [32], 96, (1, 1), 1, (0, 0), 3, 85, 20, {'EEM_GCONVB_1X1': '1'}),
    ('gconvb_1x1_th6', [32], 96, (1, 1), 1, (0, 0), 3, 169, 20, {'EEM_GCONVB_1X1': '1'}),
    ('gconvb_1x1_th8', [32], 192, (1, 1), 1, (0, 0), 3, 127, 20, {'EEM_GCONVB_1X1': '1'}),
    ('gconvb_3x3_th2', [32], 128, (3, 3), 1, (1, 1), 1, 7, 20, {'EEM_GCONVB_MINBLK': '1'}),
    ('gconvb_3x3_th4', [32], 96, (3, 3), 1, (1, 1), 3, 85, 20, {}),
    ('gconvb_3x3_th6', [32], 96, (3, 3), 1, (1, 1), 3, 169, 20, {}),
    ('gconvb_3x3_th8', [32], 96, (3, 3), 1, (1, 1), 3, 253, 20, {}),
    ('gconvb_1x5_th2', [32], 192, (1, 5), 1, (0, 2), 1, 7, 20, {'EEM_GCONVB_MINBLK': '1'}),
    ('gconvb_1x5_th4', [32], 128, (1, 5), 1, (0, 2), 3, 85, 20, {}),
    ('gconvb_1x5_th6', [32], 96, (1, 5), 1, (0, 2), 3, 169, 20, {}),
    ('gconvb_1x5_th8', [32], 96, (1, 5), 1, (0, 2), 3, 253, 20, {}),
    ('gconvb_5x1_th2', [32], 96, (5, 1), 1, (2, 0), 1, 7, 20, {'EEM_GCONVB_MINBLK': '1'}),
    ('gconvb_5x1_th4', [32], 192, (5, 1), 1, (2, 0), 3, 43, 20, {}),
    ('gconvb_5x1_th6', [32], 128, (5, 1), 1, (2, 0), 3, 169, 20, {}),
    ('gconvb_5x1_th8', [32], 96, (5, 1), 1, (2, 0), 3, 253, 20, {}),
    ('gconvb_1x1_th2', [64, 32], 128, (1, 1), 1, (0, 0), 2, 7, 20, {'EEM_GCONVB_1X1': '1', 'EEM_GCONVB_MINBLK': '1'}),
    ('gconvb_3x3_th2', [64, 32], 128, (3, 3), 1, (1, 1), 2, 7, 20, {'EEM_GCONVB_MINBLK': '1'}),
    ('gconvb_1x5_th2', [64, 32], 128, (1, 5), 1, (0, 2), 2, 7, 20, {'EEM_GCONVB_MINBLK': '1'}),
    ('gconvb_5x1_th2', [64, 32], 128, (5, 1), 1, (2, 0), 2, 7, 20, {'EEM_GCONVB_MINBLK': '1'}),
    ('generic_splitk16', [120], 64, (3, 3), 1, (1, 1), 2, 15, 19, {}),
    ('gconv16_1x5_th2_wm4_kg2', [128, 128, 128], 128, (1, 5), 1, (0, 2), 2, 30, 40, {'EEM_NO_GCONVB': '1'}),
    ('gconv16_5x1_th2_wm4_kg2', [128, 128, 128], 96, (5, 1), 1, (2, 0), 1, 50, 72, {'EEM_NO_GCONVB': '1'}),
    ('gconv16_3x3_th2_wm4_kg2', [336], 192, (3, 3), 1, (1, 1), 1, 26, 36, {}),
    ('gconv16_3x3_th2_wm4_kg2', [32, 32, 16], 64, (3, 3), 1, (1, 1), 2, 30, 44, {}),
    ('gconv16_3x3_s2', [64], 128, (3, 3), 2, (1, 1), 2, 91, 136, {}),
    ('gconv16_1x1_s2', [96], 80, (1, 1), 2, (0, 0), 2, 91, 136, {}),
    ('generic_splitk4', [64], 128, (3, 3), 2, (1, 1), 2, 91, 136, {'EEM_NO_G16_S2': '1'}),
    ('gconvb_1x5_th4', [128, 128, 128], 128, (1, 5), 1, (0, 2), 2, 60, 80, {}),
    ('gconvb_5x1_th4', [128, 128, 128], 256, (5, 1), 1, (2, 0), 1, 60, 80, {}),
    ('gconv16_3x3_th3_wm4_kg2', [128], 128, (3, 3), 1, (1, 1), 1, 61, 84, {}),
    ('taps_7x7', [1], 32, (7, 7), 2, (3, 3), 2, 45, 52, {}),
    ('taps_7x7', [2], 96, (7, 7), 2, (3, 3), 1, 50, 67, {}),
    ('taps_7x7', [5], 64, (7, 7), 2, (3, 3), 2, 45, 52, {}),
    ('taps_7x7', [6], 40, (7, 7), 2, (3, 3), 1, 37, 50, {}),
    ('taps_7x7', [3], 64, (7, 7), 2, (3, 3), 2, 44, 60, {}),
    ('taps_7x7', [4], 64, (7, 7), 2, (3, 3), 1, 45, 52, {}),
    ('taps_3x3', [1], 48, (3, 3), 1, (1, 1), 2, 37, 45, {}),
    ('taps_3x3', [2], 16, (3, 3), 1, (1, 1), 1, 50, 67, {}),
    ('fewout_wide2', [256], 2, (3, 3), 1, (1, 1), 2, 30, 41, {}),
    ('fewout_wide2', [100], 1, (3, 3), 1, (1, 1), 1, 33, 47, {}),
    ('fewout_k16_c2', [300], 2, (3, 3), 1, (1, 1), 1, 33, 47, {}),
    ('fewout_k8_c2', [32], 2, (3, 3), 1, (1, 1), 1, 64, 65, {}),
    ('fewout_k8_c2', [64], 1, (3, 3), 1, (1, 1), 2, 70, 99, {}),
    ('fewout_k8_c4', [24], 3, (3, 3), 1, (1, 1), 2, 31, 45, {}),
    ('fewout_k8_c4', [67], 4, (3, 3), 1, (1, 1), 2, 130, 131, {}),
    ('fewout_k16_c8', [176], 8, (3, 3), 1, (1, 1), 2, 37, 45, {}),
    ('fewout_k16_c8', [100], 3, (3, 3), 1, (1, 1), 1, 33, 47, {}),
    ('fewout_k8_c8', [24], 5, (3, 3), 1, (1, 1), 2, 31, 45, {}),
    ('fewout_k8_c8', [80], 8, (3, 3), 1, (1, 1), 2, 130, 131, {}),
    ('generic_2x2_b1', [1], 40, (1, 5), 1, (0, 2), 2, 257, 262, {}),
    ('generic_2x2_b4', [5], 48, (3, 3), 1, (1, 1), 2, 258, 259, {}),
    ('generic_1x1_b1', [2], 24, (1, 1), 1, (0, 0), 2, 37, 45, {}),
    ('generic_1x1_b4', [8], 33, (3, 3), 1, (1, 1), 3, 31, 45, {}),
    ('generic_2x2', [10], 64, (3, 3), 1, (1, 1), 2, 258, 259, {}),
    ('generic_2x1', [12], 20, (3, 3), 1, (1, 1), 2, 258, 259, {}),
    ('generic_1x1', [10], 24, (1, 1), 1, (0, 0), 2, 37, 45, {}),
    ('generic_splitk16', [128], 64, (3, 3), 1, (1, 1), 1, 20, 20, {}),
    ('generic_splitk8', [72], 64, (3, 3), 1, (1, 1), 1, 30, 37, {}),
    ('generic_splitk4', [72], 64, (3, 3), 1, (1, 1), 2, 45, 53, {}),
    ('generic_splitk8', [256], 2, (3, 3), 1, (1, 1), 2, 30, 41, {'EEM_NO_FEWOUT': '1'}),
    ('generic_splitk4', [128], 128, (3, 3), 1, (1, 1), 1, 50, 71, {}),
    ('generic_splitk4', [128, 128], 128, (1, 5), 1, (0, 2), 2, 30, 42, {}),
    ('generic_1x1', [64], 64, (3, 3), 1, (1, 1), 1, 40, 52, {'EEM_NO_GCONV16': '1', 'EEM_NO_SPLITK': '1'}),
    ('generic_splitk8', [64], 64, (3, 3), 1, (0, 0), 2, 30, 44, {}),
]
# (form, cin, ci0, cic, cout, (kh, kw), stride, (ph, pw), n, h, w, switches)
DGRAD = [
    ('gconv16_3x3_th2_wm4_kg2', 64, 0, 64, 80, (3, 3), 1, (1, 1), 2, 30, 44, {}),
    ('gconv16_3x3_th3_wm4_kg2', 128, 0, 128, 128, (3, 3), 1, (1, 1), 1, 61, 84, {}),
    ('gconvb_1x5_th2', 128, 0, 128, 128, (1, 5), 1, (0, 2), 2, 30, 40, {'EEM_GCONVB_MINBLK': '1'}),
    ('gconv16_1x5_th2_wm4_kg2', 384, 128, 128, 128, (1, 5), 1, (0, 2), 2, 30, 40, {}),
    ('gconv16_5x1_th2_wm4_kg2', 384, 256, 128, 96, (5, 1), 1, (2, 0), 2, 30, 44, {'EEM_NO_GCONVB': '1'}),
    ('fewout_k16_c8', 3, 0, 3, 64, (3, 3), 1, (1, 1), 2, 31, 45, {}),
    ('fewout_k8_c8', 8, 0, 8, 80, (3, 3), 1, (1, 1), 2, 130, 131, {}),
    ('taps_3x3', 256, 0, 256, 2, (3, 3), 1, (1, 1), 2, 30, 41, {}),
    ('generic_1x1', 10, 0, 10, 24, (3, 3), 1, (1, 1), 2, 37, 45, {}),
    ('generic_splitk8', 72, 0, 72, 64, (3, 3), 1, (1, 1), 1, 30, 37, {}),
    ('gconv16_1x1_th2_wm4_kg2', 128, 0, 128, 64, (1, 1), 1, (0, 0), 2, 30, 44, {}),
    ('generic_splitk4', 100, 30, 50, 72, (1, 5), 1, (0, 2), 1, 30, 41, {}),
    ('dgrad_s2w_96_3x3', 64, 0, 64, 96, (3, 3), 2, (1, 1), 2, 91, 136, {}),
    ('dgrad_s2w_128_3x3', 96, 0, 96, 128, (3, 3), 2, (1, 1), 2, 90, 136, {}),
    ('dgrad_s2w_96_1x1', 64, 0, 64, 96, (1, 1), 2, (0, 0), 2, 90, 136, {}),
    ('dgrad_s2w_128_1x1', 96, 0, 96, 128, (1, 1), 2, (0, 0), 2, 91, 136, {}),
    ('dgrad_t2_generic_splitk4', 64, 0, 64, 128, (3, 3), 2, (1, 1), 2, 91, 136, {'EEM_NO_DGRAD_S2W': '1'}),
    ('dgrad_t2_generic_splitk4', 32, 0, 32, 64, (3, 3), 2, (1, 1), 2, 91, 136, {}),
    ('dgrad_t2_generic_splitk4', 64, 0, 64, 128, (3, 3), 2, (1, 1), 2, 90, 135, {}),
    ('dgrad_t2_generic_2x2', 64, 0, 64, 64, (1, 1), 2, (0, 0), 2, 258, 259, {}),
    ('dgrad_t2_generic_2x1', 24, 0, 24, 64, (1, 1), 2, (0, 0), 4, 258, 259, {}),
    ('dgrad_t2_generic_1x1', 24, 0, 24, 64, (1, 1), 2, (0, 0), 2, 180, 200, {}),
    ('dgrad_t2_generic_splitk8', 64, 0, 64, 128, (3, 3), 2, (1, 1), 2, 30, 37, {}),
    ('dgrad_t2_generic_splitk16', 64, 0, 64, 128, (3, 3), 2, (1, 1), 1, 22, 27, {}),
    ('dgrad_t2_generic_splitk16', 64, 0, 64, 128, (3, 3), 2, (1, 1), 2, 15, 19, {}),
    ('dgrad_t2_generic_2x2_b1', 40, 0, 40, 2, (3, 3), 2, (1, 1), 2, 258, 259, {}),
    ('dgrad_t2_generic_2x2_b4', 40, 0, 40, 8, (3, 3), 2, (1, 1), 2, 258, 259, {}),
    ('dgrad_t2_generic_1x1_b1', 24, 0, 24, 2, (3, 3), 2, (1, 1), 2, 180, 200, {}),
    ('dgrad_t2_generic_1x1_b4', 24, 0, 24, 8, (3, 3), 2, (1, 1), 2, 180, 200, {}),
    ('dgrad_t2_generic_2x1', 5, 0, 5, 64, (7, 7), 2, (3, 3), 4, 321, 328, {}),
    ('dgrad_t2_generic_2x1', 3, 0, 3, 64, (7, 7), 2, (3, 3), 2, 400, 419, {}),
]
# (form, input segments, cout, (kh, kw), stride, (ph, pw), n, h, w, switches, one call over the segments, ci0, dw's cin)
WGRAD = [
    ('wgrad_ring_s2_6464', [64], 128, (3, 3), 2, (1, 1), 2, 91, 136, {}, False, 0, 64),
    ('wgrad_ring_s2_6464', [96], 80, (3, 3), 2, (1, 1), 2, 89, 136, {}, False, 0, 96),
    ('wgrad_ring_s2_6432', [32], 64, (3, 3), 2, (1, 1), 2, 91, 136, {'EEM_WGRAD_RING': 'all'}, False, 0, 32),
    ('wgrad_ring_s2_3216', [16], 32, (3, 3), 2, (1, 1), 2, 91, 136, {'EEM_WGRAD_RING': 'all'}, False, 0, 16),
    ('wgrad_ring_6464', [80], 96, (3, 3), 1, (1, 1), 2, 30, 44, {'EEM_WGRAD_RING': 'all'}, False, 0, 80),
    ('wgrad_ring_3232', [32], 32, (3, 3), 1, (1, 1), 2, 30, 44, {'EEM_WGRAD_RING': 'all'}, False, 0, 32),
    ('wgrad_ring_1616', [16], 16, (3, 3), 1, (1, 1), 2, 30, 44, {'EEM_WGRAD_RING': 'all'}, False, 0, 16),
    ('wgrad_ring_wide_1x5', [80], 96, (1, 5), 1, (0, 2), 2, 30, 44, {'EEM_WGRAD_RING': 'all'}, False, 0, 80),
    ('wgrad_ring_wide_5x1_6464', [80], 96, (5, 1), 1, (2, 0), 2, 30, 44, {'EEM_WGRAD_RING': 'all'}, False, 0, 80),
    ('wgrad_ring_wide_5x1_6432', [80], 96, (5, 1), 1, (2, 0), 2, 30, 84, {'EEM_WGRAD_RING': 'all'}, False, 0, 80),
    ('wgrad_ring_wide_1x5_cat2', [128, 128], 128, (1, 5), 1, (0, 2), 2, 30, 40, {'EEM_WGRAD_RING': 'all'}, True, 0, 256),
    ('wgrad_ring_wide_5x1_6464_cat2', [128, 128], 96, (5, 1), 1, (2, 0), 2, 30, 40, {'EEM_WGRAD_RING': 'all'}, True, 0, 256),
    ('wgrad_ring_6464_cat2', [128, 128], 96, (3, 3), 1, (1, 1), 2, 30, 40, {'EEM_WGRAD_RING': 'all'}, True, 0, 256),
    ('wgrad_ring_wide_1x5_cat3', [128, 128, 128], 128, (1, 5), 1, (0, 2), 2, 30, 40, {'EEM_WGRAD_RING': 'all'}, True, 0, 384),
    ('wgrad_ring_wide_5x1_6464_cat3', [128, 128, 128], 96, (5, 1), 1, (2, 0), 2, 30, 40, {'EEM_WGRAD_RING': 'all'}, True, 0, 384),
    ('wgrad_ring_6464_cat3', [128, 128, 128], 96, (3, 3), 1, (1, 1), 2, 30, 40, {'EEM_WGRAD_RING': 'all'}, True, 0, 384),
    ('wgrad_ring_wide_1x5_cat2', [48, 20], 80, (1, 5), 1, (0, 2), 2, 21, 36, {'EEM_WGRAD_RING': 'all'}, True, 0, 68),
    ('wgrad_ring_wide_5x1_6464_cat2', [48, 20], 96, (5, 1), 1, (2, 0), 2, 21, 36, {'EEM_WGRAD_RING': 'all'}, True, 0, 68),
    ('wgrad_ring_6464_cat2', [48, 20], 96, (3, 3), 1, (1, 1), 2, 21, 36, {'EEM_WGRAD_RING': 'all'}, True, 0, 68),
    ('wgrad_ring_wide_1x5_cat3', [40, 24, 16], 80, (1, 5), 1, (0, 2), 2, 21, 36, {'EEM_WGRAD_RING': 'all'}, True, 0, 80),
    ('wgrad_ring_wide_5x1_6464_cat3', [40, 24, 16], 96, (5, 1), 1, (2, 0), 2, 21, 36, {'EEM_WGRAD_RING': 'all'}, True, 0, 80),
    ('wgrad_ring_6464_cat3', [40, 24, 16], 96, (3, 3), 1, (1, 1), 2, 21, 36, {'EEM_WGRAD_RING': 'all'}, True, 0, 80),
    ('wgrad_ring_wide_5x1_6432_cat2', [48, 20], 96, (5, 1), 1, (2, 0), 2, 21, 84, {'EEM_WGRAD_RING': 'all'}, True, 0, 68),
    ('wgrad_ring_wide_5x1_6432_cat3', [40, 24, 16], 96, (5, 1), 1, (2, 0), 2, 21, 84, {'EEM_WGRAD_RING': 'all'}, True, 0, 80),
    ('wgrad_ring_s2_6464_cat2', [48, 32], 80, (3, 3), 2, (1, 1), 2, 43, 72, {}, True, 0, 80),
    ('wgrad_ring_s2_6464_cat3', [32, 32, 16], 80, (3, 3), 2, (1, 1), 2, 43, 72, {}, True, 0, 80),
    ('wgrad_ring_s2_6432_cat2', [16, 16], 64, (3, 3), 2, (1, 1), 2, 43, 72, {'EEM_WGRAD_RING': 'all'}, True, 0, 32),
    ('wgrad_ring_3232_cat2', [16, 16], 32, (3, 3), 1, (1, 1), 2, 21, 36, {'EEM_WGRAD_RING': 'all'}, True, 0, 32),
    ('wgrad_ring_s2_6432_cat3', [16, 8, 8], 64, (3, 3), 2, (1, 1), 2, 43, 72, {'EEM_WGRAD_RING': 'all'}, True, 0, 32),
    ('wgrad_ring_3232_cat3', [16, 8, 8], 32, (3, 3), 1, (1, 1), 2, 21, 36, {'EEM_WGRAD_RING': 'all'}, True, 0, 32),
    ('wgrad_ring_s2_3216_cat2', [8, 8], 32, (3, 3), 2, (1, 1), 2, 43, 72, {'EEM_WGRAD_RING': 'all'}, True, 0, 16),
    ('wgrad_ring_1616_cat2', [8, 8], 16, (3, 3), 1, (1, 1), 2, 21, 36, {'EEM_WGRAD_RING': 'all'}, True, 0, 16),
    ('wgrad_ring_s2_3216_cat3', [8, 4, 4], 32, (3, 3), 2, (1, 1), 2, 43, 72, {'EEM_WGRAD_RING': 'all'}, True, 0, 16),
    ('wgrad_ring_1616_cat3', [8, 4, 4], 16, (3, 3), 1, (1, 1), 2, 21, 36, {'EEM_WGRAD_RING': 'all'}, True, 0, 16),
    ('wgrad_wide_bx3_tw16_1x5+wgrad_wide_bx3_tw16_1x5+wgrad_wide_bx3_tw16_1x5', [128, 128, 128], 128, (1, 5), 1, (0, 2), 2, 30, 40, {}, True, 0, 384),
    ('wgrad_enc_bx3_tw16_c64_s1+wgrad_enc_bx3_tw16_c64_s1', [64, 32], 64, (3, 3), 1, (1, 1), 2, 30, 44, {}, True, 0, 96),
    ('wgrad_enc_fp32_tw16_c64_s1+wgrad_enc_fp32_tw16_c64_s1', [64, 32], 64, (3, 3), 1, (1, 1), 2, 30, 44, {'EEM_NO_WGRAD_BX3': '1'}, True, 0, 96),
    ('wgrad_generic_3x3_s1_bias+wgrad_generic_3x3_s1', [48, 24], 72, (3, 3), 1, (1, 1), 2, 10, 11, {}, True, 0, 72),
    ('wgrad_few_c2', [512], 2, (3, 3), 1, (1, 1), 1, 9, 13, {}, False, 0, 512),
    ('wgrad_few_c2', [700], 1, (3, 3), 1, (1, 1), 2, 7, 9, {}, False, 0, 700),
    ('wgrad_few_c4', [400], 4, (3, 3), 1, (1, 1), 2, 9, 11, {}, False, 0, 400),
    ('wgrad_few_c4', [367], 3, (3, 3), 1, (1, 1), 1, 9, 13, {}, False, 0, 367),
    ('wgrad_few_c8', [300], 8, (3, 3), 1, (1, 1), 2, 11, 13, {}, False, 0, 300),
    ('wgrad_few_c8', [250], 5, (3, 3), 1, (1, 1), 1, 11, 13, {}, False, 0, 250),
    ('wgrad_enc_fp32_tw16_c16_s1', [16], 16, (3, 3), 1, (1, 1), 2, 30, 44, {}, False, 0, 16),
    ('wgrad_enc_fp32_tw32_c16_s1', [16], 16, (3, 3), 1, (1, 1), 2, 30, 64, {}, False, 0, 16),
    ('wgrad_enc_fp32_tw16_c16_s2', [5], 16, (3, 3), 2, (1, 1), 2, 59, 88, {}, False, 0, 5),
    ('wgrad_enc_fp32_tw32_c5_c16_s2', [5], 16, (3, 3), 2, (1, 1), 2, 6, 128, {}, False, 0, 5),
    ('wgrad_enc_bx3_tw16_c32_s1', [48], 32, (3, 3), 1, (1, 1), 2, 30, 44, {}, False, 0, 48),
    ('wgrad_enc_fp32_tw16_c32_s1', [48], 32, (3, 3), 1, (1, 1), 2, 30, 44, {'EEM_NO_WGRAD_BX3': '1'}, False, 0, 48),
    ('wgrad_enc_bx3_tw32_c32_s1', [48], 32, (3, 3), 1, (1, 1), 2, 30, 64, {}, False, 0, 48),
    ('wgrad_enc_fp32_tw32_c32_s1', [48], 32, (3, 3), 1, (1, 1), 2, 30, 64, {'EEM_NO_WGRAD_BX3': '1'}, False, 0, 48),
    ('wgrad_enc_bx3_tw16_c32_s2', [16], 32, (3, 3), 2, (1, 1), 2, 59, 88, {}, False, 0, 16),
    ('wgrad_enc_fp32_tw16_c32_s2', [16], 32, (3, 3), 2, (1, 1), 2, 59, 88, {'EEM_NO_WGRAD_BX3': '1'}, False, 0, 16),
    ('wgrad_enc_bx3_tw32_c32_s2', [16], 32, (3, 3), 2, (1, 1), 2, 59, 128, {}, False, 0, 16),
    ('wgrad_enc_fp32_tw32_c32_s2', [16], 32, (3, 3), 2, (1, 1), 2, 59, 128, {'EEM_NO_WGRAD_BX3': '1'}, False, 0, 16),
    ('wgrad_enc_bx3_tw16_c64_s1', [32], 64, (3, 3), 1, (1, 1), 2, 30, 44, {}, False, 0, 32),
    ('wgrad_enc_fp32_tw16_c64_s1', [32], 64, (3, 3), 1, (1, 1), 2, 30, 44, {'EEM_NO_WGRAD_BX3': '1'}, False, 0, 32),
    ('wgrad_enc_bx3_tw32_c64_s1', [32], 64, (3, 3), 1, (1, 1), 2, 30, 64, {}, False, 0, 32),
    ('wgrad_enc_fp32_tw32_c64_s1', [32], 64, (3, 3), 1, (1, 1), 2, 30, 64, {'EEM_NO_WGRAD_BX3': '1'}, False, 0, 32),
    ('wgrad_enc_bx3_tw16_c64_s2', [32], 64, (3, 3), 2, (1, 1), 2, 59, 88, {}, False, 0, 32),
    ('wgrad_enc_fp32_tw16_c64_s2', [32], 64, (3, 3), 2, (1, 1), 2, 59, 88, {'EEM_NO_WGRAD_BX3': '1'}, False, 0, 32),
    ('wgrad_enc_bx3_tw32_c64_s2', [32], 64, (3, 3), 2, (1, 1), 2, 59, 128, {}, False, 0, 32),
    ('wgrad_enc_fp32_tw32_c64_s2', [32], 64, (3, 3), 2, (1, 1), 2, 59, 128, {'EEM_NO_WGRAD_BX3': '1'}, False, 0, 32),
    ('wgrad_wide_bx3_tw16_3x3', [48], 80, (3, 3), 1, (1, 1), 2, 30, 44, {}, False, 0, 48),
    ('wgrad_wide_fp32_tw16_3x3', [48], 80, (3, 3), 1, (1, 1), 2, 30, 44, {'EEM_NO_WGRAD_BX3': '1'}, False, 0, 48),
    ('wgrad_wide_bx3_tw32_3x3', [48], 80, (3, 3), 1, (1, 1), 2, 30, 64, {}, False, 0, 48),
    ('wgrad_wide_fp32_tw32_3x3', [48], 80, (3, 3), 1, (1, 1), 2, 30, 64, {'EEM_NO_WGRAD_BX3': '1'}, False, 0, 48),
    ('wgrad_wide_bx3_tw16_1x5', [48], 80, (1, 5), 1, (0, 2), 2, 30, 44, {}, False, 0, 48),
    ('wgrad_wide_fp32_tw16_1x5', [48], 80, (1, 5), 1, (0, 2), 2, 30, 44, {'EEM_NO_WGRAD_BX3': '1'}, False, 0, 48),
    ('wgrad_wide_bx3_tw32_1x5', [48], 80, (1, 5), 1, (0, 2), 2, 30, 64, {}, False, 0, 48),
    ('wgrad_wide_fp32_tw32_1x5', [48], 80, (1, 5), 1, (0, 2), 2, 30, 64, {'EEM_NO_WGRAD_BX3': '1'}, False, 0, 48),
    ('wgrad_wide_bx3_tw16_5x1', [48], 80, (5, 1), 1, (2, 0), 2, 30, 44, {}, False, 0, 48),
    ('wgrad_wide_fp32_tw16_5x1', [48], 80, (5, 1), 1, (2, 0), 2, 30, 44, {'EEM_NO_WGRAD_BX3': '1'}, False, 0, 48),
    ('wgrad_wide_bx3_tw32_5x1', [48], 80, (5, 1), 1, (2, 0), 2, 30, 64, {}, False, 0, 48),
    ('wgrad_wide_fp32_tw32_5x1', [48], 80, (5, 1), 1, (2, 0), 2, 30, 64, {'EEM_NO_WGRAD_BX3': '1'}, False, 0, 48),
    ('wgrad_wide_bx3_tw16_1x1', [48], 80, (1, 1), 1, (0, 0), 2, 30, 44, {}, False, 0, 48),
    ('wgrad_wide_fp32_tw16_1x1', [48], 80, (1, 1), 1, (0, 0), 2, 30, 44, {'EEM_NO_WGRAD_BX3': '1'}, False, 0, 48),
    ('wgrad_wide_bx3_tw32_1x1', [48], 80, (1, 1), 1, (0, 0), 2, 30, 64, {}, False, 0, 48),
    ('wgrad_wide_fp32_tw32_1x1', [48], 80, (1, 1), 1, (0, 0), 2, 30, 64, {'EEM_NO_WGRAD_BX3': '1'}, False, 0, 48),
    ('wgrad_wide_bx3_tw16_3x3', [128], 128, (3, 3), 1, (1, 1), 1, 50, 72, {}, False, 0, 128),
    ('wgrad_enc_fp32_tw32_c16_s2', [16], 16, (3, 3), 2, (1, 1), 2, 59, 128, {}, False, 0, 16),
    ('wgrad_wide_bx3_tw16_1x5', [128], 128, (1, 5), 1, (0, 2), 2, 30, 40, {}, False, 128, 384),
    ('wgrad_ring_6464', [48], 80, (3, 3), 1, (1, 1), 2, 30, 44, {'EEM_WGRAD_RING': 'all'}, False, 16, 70),
    ('wgrad_generic_3x3_s1_bias', [40], 72, (3, 3), 1, (1, 1), 2, 10, 11, {}, False, 5, 64),
    ('wgrad_few_c2', [400], 2, (3, 3), 1, (1, 1), 1, 9, 13, {}, False, 28, 512),
    ('wgrad_generic_3x3_s1_bias', [48], 72, (3, 3), 1, (1, 1), 2, 10, 11, {}, False, 0, 48),
    ('wgrad_generic_3x3_s1_bias', [24], 160, (3, 3), 1, (1, 1), 2, 10, 11, {}, False, 0, 24),
    ('wgrad_generic_3x3_s2_bias', [48], 72, (3, 3), 2, (1, 1), 2, 21, 23, {}, False, 0, 48),
    ('wgrad_generic_1x1_s1_bias', [200], 136, (1, 1), 1, (0, 0), 2, 10, 11, {}, False, 0, 200),
    ('wgrad_generic_1x1_s2_bias', [200], 136, (1, 1), 2, (0, 0), 2, 21, 23, {}, False, 0, 200),
    ('wgrad_generic_1x5_s1_bias', [48], 72, (1, 5), 1, (0, 2), 2, 10, 11, {}, False, 0, 48),
    ('wgrad_generic_5x1_s1_bias', [48], 72, (5, 1), 1, (2, 0), 2, 10, 11, {}, False, 0, 48),
    ('wgrad_generic_7x7_s2_bias', [5], 64, (7, 7), 2, (3, 3), 2, 16, 18, {}, False, 0, 5),
    ('wgrad_generic_7x7_s1_bias', [6], 32, (7, 7), 1, (3, 3), 2, 7, 9, {}, False, 0, 6),
]


def _ids(cases):
    return [f"{i:03d}-{c[0]}" for i, c in enumerate(cases)]


@pytest.mark.parametrize("idx", range(len(FWD)), ids=_ids(FWD))
def test_forward(monkeypatch, idx):
    form, cs, cout, k, stride, pad, n, h, w, env = FWD[idx]
    _pin(monkeypatch, env)
    g = torch.Generator().manual_seed(_seed("fwd", idx))
    wt, b = B.seeded_conv(_seed("fwd-w", idx) % 2**31, sum(cs), cout, k, stride, pad)
    xs = [torch.randn(n, c, h, w, generator=g) for c in cs]
    act, out_scale = ACTS[idx % 3], (0.25 if idx % 4 == 1 else 1.0)
    coff, ctotal = (idx % 3) * 4, cout + 8                    # (a multiple of four: the LDS-tiled kernels want their rows 16-byte aligned)
    out, ran = run_fwd(xs, wt, b if idx % 5 else None, stride, pad, act, out_scale, ctotal, coff)
    assert ran == form, f"{ran} ran, not {form}"
    SEEN.add(ran)
    RAN.add(("fwd", idx))
    rest = torch.cat([out[:, :coff], out[:, coff + cout:]], 1)
    assert torch.equal(rest, torch.full_like(rest, SENTINEL)), "channels outside [out_coff, out_coff + cout) were written"
    ref, mag = B.op_conv_ref(xs, wt, b if idx % 5 else None, stride=stride, padding=pad, act=act, out_scale=out_scale)
    B.check_form(f"fwd[{idx}] {cs}->{cout} {k[0]}x{k[1]} s{stride} {n}x{h}x{w} act {act} x{out_scale}", ran, out[:, coff:coff + cout], ref, mag,
                 tile=_tile(ran))


@pytest.mark.parametrize("idx", range(len(DGRAD)), ids=_ids(DGRAD))
def test_data_gradient(monkeypatch, idx):
    form, cin, ci0, cic, cout, k, stride, pad, n, h, w, env = DGRAD[idx]
    _pin(monkeypatch, env)
    g = torch.Generator().manual_seed(_seed("dgrad", idx))
    wt, _ = B.seeded_conv(_seed("dgrad-w", idx) % 2**31, cin, cout, k, stride, pad)
    hout, wout = (h + 2 * pad[0] - k[0]) // stride + 1, (w + 2 * pad[1] - k[1]) // stride + 1
    dy = B.random_sign((n, cout, hout, wout), g)
    ref, mag = B.op_dgrad_ref(dy, wt, (h, w), stride=stride, padding=pad, ci0=ci0, cic=cic)
    runs = []
    for rep in range(4):
        dx, ran = run_dgrad(dy, wt, (h, w), stride, pad, ci0, cic)
        assert ran == form, f"{ran} ran, not {form}"
        SEEN.add(ran)
        if rep and torch.equal(dx, runs[0]):
            break                                               # bitwise repeatable: one run is all runs
        runs.append(dx)
        B.check_form(f"dgrad[{idx}] {cin}[{ci0}:{ci0 + cic}]<-{cout} {k[0]}x{k[1]} s{stride} {n}x{h}x{w} run {rep}", ran, dx, ref, mag, tile=_tile(ran),
                     ref32=lambda: torch.nn.grad.conv2d_input((n, cic, h, w), wt[:, ci0:ci0 + cic].contiguous(), dy, stride=stride, padding=pad))
    RAN.add(("dgrad", idx))


@pytest.mark.parametrize("idx", range(len(WGRAD)), ids=_ids(WGRAD))
def test_weight_gradient(monkeypatch, idx):
    form, cs, cout, k, stride, pad, n, h, w, env, cat, ci0, cin = WGRAD[idx]
    _pin(monkeypatch, env)
    g = torch.Generator().manual_seed(_seed("wgrad", idx))
    xs = [torch.randn(n, c, h, w, generator=g) for c in cs]
    hout, wout = (h + 2 * pad[0] - k[0]) // stride + 1, (w + 2 * pad[1] - k[1]) // stride + 1
    dy = B.random_sign((n, cout, hout, wout), g)
    wshape = (cout, cin, *k)
    ref, mag, bref, bmag = B.op_wgrad_ref(xs, dy, wshape, stride=stride, padding=pad, ci0=ci0)
    # prefills of the gradients' own size: `=` for `+=` is then an error of the whole gradient, the prefill's rounding a unit of the sum's
    pre_w = torch.randn(wshape, generator=g) * float(ref.abs().mean() * (cin / sum(cs)))
    pre_b = torch.randn(cout, generator=g) * float(bref.abs().mean())
    for rep in range(4):
        with_db = rep != 3
        dw, db, ran = run_wgrad(xs, dy, wshape, stride, pad, ci0, pre_w, pre_b if with_db else None, cat)
        # (without db the batched fallback does not launch its bias-gradient kernel)
        want = form if with_db else "+".join(p[:-len("_bias")] if p.endswith("_bias") else p for p in form.split("+"))
        assert ran == want, f"{ran} ran, not {want}"
        SEEN.update(ran.split("+"))
        name = f"wgrad[{idx}] {cs}->{cout} in {cin}[{ci0}:] {k[0]}x{k[1]} s{stride} {n}x{h}x{w} run {rep}"
        # the columns outside the slice hold the prefill bitwise (ref and mag are zero there: any change is an infinite z)
        B.check_form(name + " dw", ran, dw.double() - pre_w.double(), ref, mag + pre_w.double().abs() * (mag > 0))
        outside = torch.ones(cin, dtype=torch.bool)
        outside[ci0:ci0 + sum(cs)] = False
        assert torch.equal(dw[:, outside], pre_w[:, outside]), "dw columns outside the input-channel slice were written"
        if with_db:
            B.check_form(name + " db", ran, db.double() - pre_b.double(), bref, bmag + pre_b.double().abs())
    RAN.add(("wgrad", idx))


def test_every_form_in_the_table_ran():
    """The names seen over the module against the family table: no case produced a name the table lacks (check_form would have raised
    KeyError), and - when the whole module ran - every name in the table was produced."""
    table = set(B.FORM_FAMILY) | set(B.FORM_KAPPA)
    assert SEEN <= table, sorted(SEEN - table)
    every = {("fwd", i) for i in range(len(FWD))} | {("dgrad", i) for i in range(len(DGRAD))} | {("wgrad", i) for i in range(len(WGRAD))}
    if RAN == every:
        missing = sorted(table - SEEN)
        assert not missing, f"{len(missing)} forms of the table never ran: {missing}"
    # (statically: the cases name every form of the table; a weight gradient's fourth run, without db, drops "_bias")
    named = {p for c in FWD + DGRAD + WGRAD for p in c[0].split("+")}
    named |= {f[:-len("_bias")] for f in named if f.endswith("_bias")}
    assert named == table, (sorted(table - named), sorted(named - table))
