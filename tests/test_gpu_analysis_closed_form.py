"""GPU: the stand-alone analysis bank (btk_fb_analysis: analysis512_kernel in fb_analysis512.hip, fast_analysis_kernel in fb_fast.hip,
analysis_kernel in fb_kernels.hip; csrc/fb_route.h chooses) against the float64 closed form of tests/closed_forms.py -- every stream,
channel, bin and frame of every launch, dense and shipped prototypes, integer PCM in the int16 range with a seed of its own per channel.
test_gpu_fused_closed_form.py does the same for the fused kernels, which are different code.

Each X[s, :, n, :tc] is judged as [K][T] of one channel against cf.analysis_cf; the yardstick is cf.analysis_f32 on the same samples.
Bound: closed_forms.accept with FACTOR = 4 and FLOOR = 2^-22, unchanged.  The smallest seeded fault at this shape (tap 1 of the shipped
prototype dropped, M = 2048) scores 176 x the yardstick (test_closed_forms_cpu.py).

Two families of cases have a degenerate yardstick and take the route's own factor, 1.5 x the worst ratio measured on that route
(analysis512_kernel 4.35 -> 6.5, fast_analysis_kernel 4.62 -> 6.9; the generic kernel stays at 4); every other case holds FACTOR = 4:
  * a recording of ONE sample (L = 1): every polyphase vector has a single non-zero entry, so each bin is one chain of twiddle
    products and the FFT adds nothing but exact zeros.  numpy's transform then makes two or three roundings per bin (its twiddles
    are rounded from double) and measures 7 to 10e-8, not what float32 arithmetic accumulates over log2 M passes.  The kernels go
    through the M/2-point complex transform in two register passes and the Hermitian post-pass E + W^k O, about ten rounded
    operations per bin, each good to half an ulp, and land at 3 to 4e-7 -- 4.0 to 4.6 x that yardstick, rising with log2 M.  On every
    other input the same kernels measure at most 3.6.
  * a shard of ONE bin row: the rule's maxima are then taken over T values instead of K T, and rows 0 and M/2 are plain sums that
    numpy gets to within an ulp; the very same values pass at FACTOR = 4 when the whole bin range is judged (M = 512, bin 0: 4.35).
Neither is a wrong value: a dropped tap, a frame one sample late or a row of another bin score above 150 (test_closed_forms_cpu.py),
more than 20 x these factors.

The axes: frame counts on either side of a tile and of a run of tiles (A_RUN, F_RUN), S N on either side of a multiple of 8 (the kernels
compute chan = (slot / nruns) * 8 + xcd), decimation x delay compensation, other tap counts (the MT = 0, 2, 4 instantiations of the generic
kernel), short and odd recordings, unaligned rows (the scalar load path) with a ragged last tile, frame ranges and bin shards into
row-padded output between guard bands, the int16 entry -- and the kernels behind BTK_DISABLE_ANALYSIS512 / BTK_DISABLE_SYNTHESIS512 /
BTK_DISABLE_FAST / BTK_SYN_NARROW, one child process per setting.

Kernel / yardstick ratio per case (the larger of the e_max and the e_bin ratio; worst stream, channel and chunk), MI355X:

    case (worst stream, channel, chunk)             dense  shipped
    512 r1 T=1 first frames                          2.63     1.91
    512 r1 T=15 first frames                         2.24     2.50
    512 r1 T=16 first frames                         2.24     2.50
    512 r1 T=17 first frames                         2.24     2.50
    512 r1 T=256 first frames                        2.47     2.55
    512 r1 T=257 first frames                        2.47     2.55
    512 r1 T=273 first frames                        2.47     2.55
    512 r1 T=15 whole                                2.65     2.65
    512 r1 T=16 whole                                2.23     2.41
    512 r1 T=17 whole                                2.22     2.28
    512 r1 T=256 whole                               3.21     2.34
    512 r1 T=257 whole                               2.66     2.94
    512 r1 T=273 whole                               2.74     2.39
    256 r1 T=1 first frames                          2.27     2.50
    256 r1 T=31 first frames                         2.23     2.42
    256 r1 T=32 first frames                         2.23     2.42
    256 r1 T=33 first frames                         2.23     2.42
    256 r1 T=256 first frames                        2.22     2.39
    256 r1 T=257 first frames                        2.22     2.39
    256 r1 T=289 first frames                        2.22     2.39
    256 r1 T=31 whole                                2.54     2.85
    256 r1 T=32 whole                                2.58     2.25
    256 r1 T=33 whole                                2.18     2.34
    256 r1 T=256 whole                               2.18     2.34
    256 r1 T=257 whole                               2.57     2.92
    256 r1 T=289 whole                               2.75     2.27
    1024 r1 T=1 first frames                         2.72     2.42
    1024 r1 T=15 first frames                        2.47     2.38
    1024 r1 T=16 first frames                        2.47     2.38
    1024 r1 T=17 first frames                        2.47     2.38
    1024 r1 T=128 first frames                       2.60     2.47
    1024 r1 T=129 first frames                       2.60     2.47
    1024 r1 T=145 first frames                       2.60     2.41
    1024 r1 T=15 whole                               2.35     3.02
    1024 r1 T=16 whole                               3.13     2.24
    1024 r1 T=17 whole                               2.75     2.19
    1024 r1 T=128 whole                              2.48     2.49
    1024 r1 T=129 whole                              3.00     2.37
    1024 r1 T=145 whole                              2.82     2.66
    2048 r1 T=1 first frames                         2.74     2.73
    2048 r1 T=7 first frames                         2.66     2.92
    2048 r1 T=8 first frames                         2.66     2.92
    2048 r1 T=9 first frames                         2.66     3.11
    2048 r1 T=64 first frames                        2.87     3.17
    2048 r1 T=65 first frames                        2.87     3.17
    2048 r1 T=73 first frames                        2.80     3.13
    2048 r1 T=7 whole                                2.49     2.81
    2048 r1 T=8 whole                                3.45     2.94
    2048 r1 T=9 whole                                3.52     3.06
    2048 r1 T=64 whole                               3.43     2.62
    2048 r1 T=65 whole                               2.81     2.69
    2048 r1 T=73 whole                               3.36     2.68
    64 r1 T=1 first frames                           1.77     1.49
    64 r1 T=31 first frames                          2.10     1.68
    64 r1 T=32 first frames                          2.10     1.68
    64 r1 T=33 first frames                          2.10     1.68
    64 r1 T=97 first frames                          2.08     2.02
    64 r1 T=31 whole                                 1.99     1.81
    64 r1 T=32 whole                                 2.13     1.84
    64 r1 T=33 whole                                 1.82     2.03
    64 r1 T=97 whole                                 2.62     2.00
    128 r1 T=1 first frames                          2.95     1.88
    128 r1 T=31 first frames                         2.09     1.93
    128 r1 T=32 first frames                         2.09     1.93
    128 r1 T=33 first frames                         2.09     1.93
    128 r1 T=97 first frames                         2.27     2.26
    128 r1 T=31 whole                                1.95     2.19
    128 r1 T=32 whole                                2.40     2.52
    128 r1 T=33 whole                                1.85     1.70
    128 r1 T=97 whole                                2.22     2.05
    512 r1 S=1 N=1                                   1.86     2.26
    512 r1 S=1 N=7                                   2.52     2.81
    512 r1 S=2 N=4                                   2.45     2.46
    512 r1 S=3 N=3                                   2.59     2.81
    512 r1 S=2 N=9                                   2.91     2.36
    256 r1 S=1 N=1                                   1.85     1.74
    256 r1 S=1 N=7                                   2.58     2.32
    256 r1 S=2 N=4                                   2.77     2.09
    256 r1 S=3 N=3                                   2.55     2.98
    256 r1 S=2 N=9                                   3.20     2.58
    1024 r1 S=1 N=1                                  2.98     2.09
    1024 r1 S=1 N=7                                  2.79     2.85
    1024 r1 S=2 N=4                                  2.97     2.73
    1024 r1 S=3 N=3                                  2.74     2.95
    1024 r1 S=2 N=9                                  2.92     3.31
    2048 r1 S=1 N=1                                  2.40     2.42
    2048 r1 S=1 N=7                                  2.84     2.86
    2048 r1 S=2 N=4                                  2.83     3.13
    2048 r1 S=3 N=3                                  3.22     3.04
    2048 r1 S=2 N=9                                  3.20     3.00
    64 r1 S=1 N=1                                    2.26     2.01
    64 r1 S=1 N=7                                    2.21     2.42
    64 r1 S=2 N=4                                    1.88     2.47
    64 r1 S=3 N=3                                    2.86     2.85
    64 r1 S=2 N=9                                    2.72     2.41
    128 r1 S=1 N=1                                   1.97     2.02
    128 r1 S=1 N=7                                   2.80     2.00
    128 r1 S=2 N=4                                   2.24     3.06
    128 r1 S=3 N=3                                   2.49     2.44
    128 r1 S=2 N=9                                   2.49     2.91
    512 m4 r0 dct0                                   2.87     2.98
    512 m4 r0 dct1                                   2.48     2.29
    512 m4 r0 dct2                                   2.43     2.85
    512 m4 r1 dct0                                   2.94     2.26
    512 m4 r1 dct1                                   2.18     2.13
    512 m4 r1 dct2                                   2.62     2.64
    512 m4 r2 dct0                                   2.48     2.77
    512 m4 r2 dct1                                   2.51     3.17
    512 m4 r2 dct2                                   2.25     2.68
    256 m4 r0 dct0                                   2.62     2.83
    256 m4 r0 dct1                                   2.38     2.30
    256 m4 r0 dct2                                   2.59     2.11
    256 m4 r1 dct0                                   2.46     2.44
    256 m4 r1 dct1                                   2.68     2.31
    256 m4 r1 dct2                                   2.30     2.23
    256 m4 r2 dct0                                   2.38     2.46
    256 m4 r2 dct1                                   2.43     2.53
    256 m4 r2 dct2                                   2.29     2.24
    128 m2 r0 dct0                                   2.47     2.08
    128 m2 r0 dct1                                   2.70     2.27
    128 m2 r0 dct2                                   2.30     2.48
    128 m2 r1 dct0                                   2.12     2.34
    128 m2 r1 dct1                                   2.34     2.41
    128 m2 r1 dct2                                   2.53     2.31
    128 m2 r2 dct0                                   2.51     2.25
    128 m2 r2 dct1                                   2.35     2.62
    128 m2 r2 dct2                                   2.19     2.34
    512 m3 r1 generic                                2.68     2.68
    256 m2 r1 generic                                2.58     2.50
    64 m4 r1 generic                                 2.43     2.49
    128 m3 r1 generic                                2.41     2.18
    512 r1 dct0 L=1                                  4.20     4.06
    512 r1 dct0 L=255                                2.17     2.76
    512 r1 dct0 L=257                                2.08     2.60
    512 r1 dct0 L=5887                               2.40     2.72
    512 r1 dct0 L=5889                               2.40     2.72
    512 r1 dct0 L=2306                               2.49     3.02
    512 r1 dct0 L=2311                               2.49     3.10
    512 r1 dct2 L=5887                               2.34     2.67
    512 r1 dct2 L=5889                               2.34     2.67
    512 r1 dct2 L=2306                               2.27     2.73
    512 r1 dct2 L=2311                               2.62     2.73
    256 r1 dct0 L=1                                  3.20     3.60
    256 r1 dct0 L=127                                2.76     2.47
    256 r1 dct0 L=129                                2.54     2.66
    256 r1 dct0 L=4991                               2.25     2.09
    256 r1 dct0 L=4993                               2.25     2.23
    256 r1 dct0 L=1154                               2.30     2.41
    256 r1 dct0 L=1159                               2.30     2.65
    256 r1 dct2 L=4991                               2.27     2.46
    256 r1 dct2 L=4993                               2.27     2.49
    256 r1 dct2 L=1154                               2.72     2.11
    256 r1 dct2 L=1159                               2.62     2.88
    1024 r1 dct0 L=1                                 4.35     3.82
    1024 r1 dct0 L=511                               2.61     2.60
    1024 r1 dct0 L=513                               2.75     2.37
    1024 r1 dct0 L=11775                             2.60     2.64
    1024 r1 dct0 L=11777                             2.90     2.64
    1024 r1 dct0 L=4610                              2.50     2.57
    1024 r1 dct0 L=4615                              2.50     2.57
    1024 r1 dct2 L=11775                             2.63     2.80
    1024 r1 dct2 L=11777                             2.63     2.62
    1024 r1 dct2 L=4610                              2.67     2.48
    1024 r1 dct2 L=4615                              2.67     2.71
    2048 r1 dct0 L=1                                 4.62     4.27
    2048 r1 dct0 L=1023                              2.72     2.81
    2048 r1 dct0 L=1025                              3.05     3.95
    2048 r1 dct0 L=15359                             3.64     3.20
    2048 r1 dct0 L=15361                             2.99     3.20
    2048 r1 dct0 L=9218                              3.21     3.00
    2048 r1 dct0 L=9223                              3.14     2.90
    2048 r1 dct2 L=15359                             3.10     2.81
    2048 r1 dct2 L=15361                             3.10     2.56
    2048 r1 dct2 L=9218                              2.95     2.92
    2048 r1 dct2 L=9223                              2.95     3.11
    64 r1 dct0 L=1                                   2.67     2.76
    64 r1 dct0 L=31                                  2.28     3.34
    64 r1 dct0 L=33                                  2.60     1.82
    64 r1 dct0 L=1247                                2.19     2.16
    64 r1 dct0 L=1249                                2.19     2.16
    64 r1 dct0 L=290                                 2.01     2.21
    64 r1 dct0 L=295                                 2.01     2.11
    64 r1 dct2 L=1247                                2.23     2.36
    64 r1 dct2 L=1249                                2.23     2.29
    64 r1 dct2 L=290                                 2.11     2.15
    64 r1 dct2 L=295                                 2.82     2.81
    128 r1 dct0 L=1                                  2.16     3.25
    128 r1 dct0 L=63                                 2.39     2.75
    128 r1 dct0 L=65                                 2.21     2.78
    128 r1 dct0 L=2495                               2.40     2.21
    128 r1 dct0 L=2497                               2.40     2.40
    128 r1 dct0 L=578                                2.50     2.14
    128 r1 dct0 L=583                                2.50     2.14
    128 r1 dct2 L=2495                               2.33     2.43
    128 r1 dct2 L=2497                               2.33     2.43
    128 r1 dct2 L=578                                2.20     2.76
    128 r1 dct2 L=583                                2.20     2.76
    512 r1 rows float32                              2.76     2.66
    512 r1 rows int16                                2.76     2.66
    256 r1 rows float32                              2.60     2.33
    256 r1 rows int16                                2.60     2.33
    1024 r1 rows float32                             3.16     3.15
    1024 r1 rows int16                               3.16     3.15
    512 r1 ranges                                    3.05     2.74
    256 r1 ranges                                    3.59     3.25
    1024 r1 ranges                                   3.06     2.80
    2048 r1 ranges                                   3.54     3.25
    64 r1 ranges                                     2.86     2.43
    128 r1 ranges                                    2.95     2.80
    512 r1 bins [0, 1)                               4.35     2.17
    512 r1 bins [256, 257)                           2.36     2.10
    512 r1 bins [85, 92)                             2.49     2.17
    512 r1 bins [128, 257)                           2.37     2.10
    1024 r1 bins [0, 1)                              2.27     2.08
    1024 r1 bins [512, 513)                          3.14     3.11
    1024 r1 bins [171, 178)                          2.32     2.67
    1024 r1 bins [256, 513)                          2.78     2.80
    64 r1 bins [0, 1)                                1.54     1.58
    64 r1 bins [32, 33)                              1.79     1.84
    64 r1 bins [11, 18)                              2.35     2.23
    64 r1 bins [16, 33)                              1.91     2.40
    512 r1 float32 entry                             2.34     3.47
    512 r1 int16 entry                               2.34     3.47
    256 r1 float32 entry                             2.54     2.65
    256 r1 int16 entry                               2.54     2.65
    1024 r1 float32 entry                            3.17     2.79
    1024 r1 int16 entry                              3.17     2.79
    2048 r1 float32 entry                            3.21     2.74
    2048 r1 int16 entry                              3.21     2.74

    The switch children (dense prototype; -A512: BTK_DISABLE_ANALYSIS512 + BTK_DISABLE_SYNTHESIS512, -FAST: BTK_DISABLE_FAST,
    -both: all three, narrow: BTK_SYN_NARROW; a dash: that setting's tile sizes give the case another T):

    case                                            -A512  -FAST  -both narrow
    512 r1 T=1 first frames                          2.67   2.63   2.77   2.63
    512 r1 T=15 first frames                         2.02   2.24   2.39   2.24
    512 r1 T=16 first frames                         2.02   2.24   2.39   2.24
    512 r1 T=17 first frames                         2.53   2.24   2.39   2.24
    512 r1 T=128 first frames                        3.06      -      -      -
    512 r1 T=129 first frames                        3.06      -      -      -
    512 r1 T=145 first frames                        3.06      -      -      -
    512 r1 T=15 whole                                2.73   2.65   2.57   2.65
    512 r1 T=16 whole                                2.77   2.23   3.04   2.23
    512 r1 T=17 whole                                2.74   2.22   2.66   2.22
    512 r1 T=128 whole                               2.68      -      -      -
    512 r1 T=129 whole                               2.43      -      -      -
    512 r1 T=145 whole                               2.30      -      -      -
    512 r1 S=1 N=1                                   2.09   1.86   2.20   1.86
    512 r1 S=1 N=7                                   2.63   2.52   2.74   2.52
    512 r1 S=2 N=4                                   2.79   2.45   2.38   2.45
    512 r1 S=3 N=3                                   2.69   2.59   2.49   2.59
    512 r1 S=2 N=9                                   2.80   2.91   3.27   2.91
    256 r1 T=1 first frames                          2.27   2.03   2.03   2.27
    256 r1 T=31 first frames                         2.23   2.03   2.03   2.23
    256 r1 T=32 first frames                         2.23   2.03   2.03   2.23
    256 r1 T=33 first frames                         2.23   2.03   2.03   2.23
    256 r1 T=256 first frames                        2.22      -      -   2.22
    256 r1 T=257 first frames                        2.22      -      -   2.22
    256 r1 T=289 first frames                        2.22      -      -   2.22
    256 r1 T=31 whole                                2.54   2.40   2.40   2.54
    256 r1 T=32 whole                                2.58   2.69   2.69   2.58
    256 r1 T=33 whole                                2.18   3.62   3.62   2.18
    256 r1 T=256 whole                               2.18      -      -   2.18
    256 r1 T=257 whole                               2.57      -      -   2.57
    256 r1 T=289 whole                               2.75      -      -   2.75
    256 r1 S=1 N=1                                   1.85   1.85   1.85   1.85
    256 r1 S=1 N=7                                   2.58   2.32   2.32   2.58
    256 r1 S=2 N=4                                   2.77   2.64   2.64   2.77
    256 r1 S=3 N=3                                   2.55   2.92   2.92   2.55
    256 r1 S=2 N=9                                   3.20   3.06   3.06   3.20
    1024 r1 T=1 first frames                         2.72   2.63   2.63   2.72
    1024 r1 T=15 first frames                        2.47      -      -   2.47
    1024 r1 T=16 first frames                        2.47      -      -   2.47
    1024 r1 T=17 first frames                        2.47      -      -   2.47
    1024 r1 T=128 first frames                       2.60      -      -   2.60
    1024 r1 T=129 first frames                       2.60      -      -   2.60
    1024 r1 T=145 first frames                       2.60      -      -   2.60
    1024 r1 T=15 whole                               2.35      -      -   2.35
    1024 r1 T=16 whole                               3.13      -      -   3.13
    1024 r1 T=17 whole                               2.75      -      -   2.75
    1024 r1 T=128 whole                              2.48      -      -   2.48
    1024 r1 T=129 whole                              3.00      -      -   3.00
    1024 r1 T=145 whole                              2.82      -      -   2.82
    1024 r1 S=1 N=1                                  2.98   1.85   1.85   2.98
    1024 r1 S=1 N=7                                  2.79   2.54   2.54   2.79
    1024 r1 S=2 N=4                                  2.97   2.34   2.34   2.97
    1024 r1 S=3 N=3                                  2.74   2.64   2.64   2.74
    1024 r1 S=2 N=9                                  2.92   2.97   2.97   2.92
    512 r1 T=256 first frames                           -   2.47      -   2.47
    512 r1 T=257 first frames                           -   2.47      -   2.47
    512 r1 T=273 first frames                           -   2.47      -   2.47
    512 r1 T=256 whole                                  -   3.21      -   3.21
    512 r1 T=257 whole                                  -   2.66      -   2.66
    512 r1 T=273 whole                                  -   2.74      -   2.74
    256 r1 T=97 first frames                            -   2.40   2.40      -
    256 r1 T=97 whole                                   -   2.62   2.62      -
    1024 r1 T=7 first frames                            -   2.30   2.30      -
    1024 r1 T=8 first frames                            -   2.30   2.30      -
    1024 r1 T=9 first frames                            -   2.30   2.30      -
    1024 r1 T=25 first frames                           -   2.33   2.33      -
    1024 r1 T=7 whole                                   -   2.44   2.44      -
    1024 r1 T=8 whole                                   -   2.37   2.37      -
    1024 r1 T=9 whole                                   -   2.42   2.42      -
    1024 r1 T=25 whole                                  -   2.47   2.47      -
    512 r1 T=49 first frames                            -      -   2.57      -
    512 r1 T=49 whole                                   -      -   2.56      -

    case (worst row spacing, piece)                 -A512  -FAST  -both narrow
    synthesis 512 m4 r0 dct2 T=19                    1.69   1.53   1.46   1.53
    synthesis 512 m4 r0 dct2 T=100                   1.72   1.64   1.71   1.64
    synthesis 512 m4 r1 dct2 T=21                    1.58   1.62   1.65   1.62
    synthesis 512 m4 r1 dct2 T=100                   2.08   1.67   1.67   1.60
    synthesis 512 m4 r2 dct1 T=32                    1.98   1.84   1.74   1.84
    synthesis 512 m4 r2 dct1 T=100                   1.69   1.61   1.84   1.61
    synthesis 256 m4 r2 dct2 T=25                    1.34   1.51   1.51   1.34
    synthesis 256 m4 r2 dct2 T=100                   1.88   1.70   1.70   1.88
    synthesis 1024 m4 r0 dct2 T=19                   1.55   1.31   1.31   1.55
    synthesis 1024 m4 r0 dct2 T=100                  1.72   1.93   1.93   1.72
    synthesis 1024 m4 r1 dct2 T=21                   1.84   1.66   1.66   1.84
    synthesis 1024 m4 r1 dct2 T=100                  2.06   1.75   1.75   2.06
    synthesis 1024 m4 r2 dct0 T=24                   1.42   1.44   1.44   1.42
    synthesis 1024 m4 r2 dct0 T=100                  1.92   1.92   1.92   1.92
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import closed_forms as cf
from tests import test_gpu_synthesis_closed_form as syn
from tests.test_gpu_synthesis_closed_form import DCT, _bank, _guarded, _proto, _same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOS = ("dense", "shipped")
GEOMS = [(512, 1), (256, 1), (1024, 1), (2048, 1), (64, 1), (128, 1)]                                  # M, r (m = 4)
BTK_SWITCHES = ("BTK_DISABLE_FUSED", "BTK_DISABLE_FAST", "BTK_DISABLE_ANALYSIS512", "BTK_DISABLE_SYNTHESIS512", "BTK_SYN_NARROW",
                "BTK_FUSED_VAR", "BTK_FUSED512_NEW")

# (route, M) -> (frames per tile, tiles a workgroup walks through)
TILES = {
    ("A512", 512): (16, 16),                                   # A_TT, A_RUN (fb_analysis512.hip)
    ("FAST", 256): (32, 8),                                    # FG<8>::TT, F_RUN (fb_fast.hip)
    ("FAST", 512): (16, 8),                                    # FG<9>::TT, F_RUN: only behind BTK_DISABLE_ANALYSIS512
    ("FAST", 1024): (16, 8),                                   # FG<10>::TT, F_RUN
    ("FAST", 2048): (8, 8),                                    # FG<11>::TT, F_RUN
}


# The rule's factor where the yardstick is degenerate (a recording of one sample, a shard of one bin row: see the module docstring):
# 1.5 x the worst ratio measured on the route.  Everywhere else, and on the generic route, it is cf.FACTOR.
ROUTE_FACTOR = {"A512": 6.5, "FAST": 6.9}


def _route(M, mm, r, off=()):
    """fb_analysis_route of csrc/fb_route.h; off: the switches that are set."""
    special = mm == 4 and r in (0, 1, 2)
    if special and M == 512 and "BTK_DISABLE_ANALYSIS512" not in off:
        return "A512"
    if special and M >= 256 and "BTK_DISABLE_FAST" not in off:
        return "FAST"
    return "GENERIC"


def _tiles(M, mm=4, r=1, off=()):
    rt = _route(M, mm, r, off)
    if rt == "GENERIC":
        return min(32, 8192 // M), None                        # FbCfg::TT (fb_kernels.hip); one tile per workgroup, no runs
    return TILES[(rt, M)]


def _degenerate_factor(M, mm=4, r=1):
    return ROUTE_FACTOR.get(_route(M, mm, r), cf.FACTOR)


def _pcm(S, N, L, seed):
    """cf.int_pcm with a seed of its own per channel: float32 [S][N][L]."""
    return np.stack([np.stack([cf.int_pcm(1, 1, L, seed=1009 * seed + 31 * s + n)[0, 0] for n in range(N)]) for s in range(S)])


def _refs(M, mm, r, dct, name, pcm):
    """Per stream and channel (closed form, float32 yardstick), each [K][T]."""
    h, K = _proto(M, mm, name), M // 2 + 1
    return [[(cf.analysis_cf(h, M, mm, r, dct, x)[:, :K].T, cf.analysis_f32(h, M, mm, r, dct, x)[:, :K].T) for x in ch] for ch in pcm]


def _judge_all(label, X, refs, t0=0, bins=None, show=True, factor=cf.FACTOR):
    """X [S][k1 - k0][N][tc] (numpy) holds the frames [t0, t0 + tc) and the bins [k0, k1): every stream and channel against the rule.
    Prints the worst channel's figures as the case's CFRATIO line and returns them."""
    S, Kx, N, tc = X.shape
    k0, k1 = bins if bins is not None else (0, Kx)
    assert (len(refs), len(refs[0]), k1 - k0) == (S, N, Kx)
    worst = None
    for s in range(S):
        for n in range(N):
            Xcf, X32 = refs[s][n]
            assert Xcf.shape[1] >= t0 + tc and Xcf.shape[0] >= k1
            fig = cf.judge("%s s=%d n=%d" % (label, s, n), X[s, :, n, :], X32[k0:k1, t0:t0 + tc], Xcf[k0:k1, t0:t0 + tc], factor, show=False)
            worst = fig if worst is None or fig["ratio"] > worst["ratio"] else worst
    if show:
        print(cf.cfratio_line(label, worst))
    return worst


def _case(dev, label, M, r, S, N, L, name, mm=4, dct=DCT, tcount=None, seed=0, i16=False, refs=None, factor=cf.FACTOR):
    """One FilterBank.analysis launch over a recording of L samples (or its first tcount frames), judged everywhere.
    -> (X numpy, refs)"""
    import torch
    fb = _bank(M, mm, r, name, dct)
    K = M // 2 + 1
    pcm = _pcm(S, N, L, seed)
    T = cf.num_frames(L, M, mm, r, dct)
    assert fb.num_frames(L) == T
    tc = T if tcount is None else tcount
    assert tc <= T
    X = fb.analysis(torch.from_numpy(pcm.astype(np.int16) if i16 else pcm).to(dev), tcount=tc).cpu().numpy()
    assert X.shape == (S, K, N, tc)
    if tc == 0:
        return X, refs
    refs = _refs(M, mm, r, dct, name, pcm) if refs is None else refs
    _judge_all(label, X, refs, factor=factor)
    return X, refs


# ---- the case lists of the frames and channels axes (the switch children run them too, with their own tile sizes) ------------
def _frames_cases(M, r, TT, RUN, mm=4, dct=DCT):
    """(tag, S, N, L, tcount, seed): every T as the first T frames of one longer recording and, from the processing delay on, as a
    recording of exactly T frames (its last tiles are zero filled past the end of the stream)."""
    Ts = [1, TT - 1, TT, TT + 1] + ([RUN * TT, RUN * TT + 1, RUN * TT + TT + 1] if RUN else [3 * TT + 1])
    pd = cf.fb_delays(mm, r, False, dct)[0]
    Llong = cf.num_samples(max(Ts) + TT + pd, M, mm, r, dct)
    out = [("T=%d first frames" % T, 1, 3, Llong, T, 1) for T in Ts]
    return out + [("T=%d whole" % T, 1, 3, cf.num_samples(T, M, mm, r, dct), None, 2 + T) for T in Ts if T >= pd]


def _channels_cases(M, r, TT, mm=4, dct=DCT):
    """S N = 1, 7, 8, 9, 18; N does not divide 8 where S > 1."""
    L = cf.num_samples(TT + 3, M, mm, r, dct)
    return [("S=%d N=%d" % (S, N), S, N, L, None, 40 + S * N) for S, N in ((1, 1), (1, 7), (2, 4), (3, 3), (2, 9))]


def _run_cases(dev, M, r, name, cases):
    shared = {}                                                # the long recording of the frames axis: one reference for all its T
    for tag, S, N, L, tcount, seed in cases:
        _, refs = _case(dev, "%d r%d %s %s" % (M, r, tag, name), M, r, S, N, L, name, tcount=tcount, seed=seed, refs=shared.get((S, N, L, seed)))
        shared = {(S, N, L, seed): refs}


@pytest.mark.parametrize("name", PROTOS)
@pytest.mark.parametrize("M,r", GEOMS)
def test_frames(dev, M, r, name):
    TT, RUN = _tiles(M, 4, r)
    assert _bank(M, 4, r, name).analysis_i16() == (RUN is not None)              # the library routes as the table above assumes
    _run_cases(dev, M, r, name, _frames_cases(M, r, TT, RUN))


@pytest.mark.parametrize("name", PROTOS)
@pytest.mark.parametrize("M,r", GEOMS)
def test_channels(dev, M, r, name):
    _run_cases(dev, M, r, name, _channels_cases(M, r, _tiles(M, 4, r)[0]))


@pytest.mark.parametrize("name", PROTOS)
@pytest.mark.parametrize("dct", [0, 1, 2])
@pytest.mark.parametrize("r", [0, 1, 2])
@pytest.mark.parametrize("M,mm", [(512, 4), (256, 4), (128, 2)])
def test_decimation_and_delay_compensation(dev, M, mm, r, dct, name):
    TT = _tiles(M, mm, r)[0]
    L = cf.num_samples(2 * TT + 1, M, mm, r, dct)
    _case(dev, "%d m%d r%d dct%d %s" % (M, mm, r, dct, name), M, r, 2, 3, L, name, mm=mm, dct=dct, seed=60 + 3 * r + dct)


@pytest.mark.parametrize("name", PROTOS)
@pytest.mark.parametrize("M,mm", [(512, 3), (256, 2), (64, 4), (128, 3)])
def test_other_tap_counts_through_the_generic_kernel(dev, M, mm, name):
    """m = 2 and m = 4 have their taps in registers (MT = 2, 4), m = 3 is the run-time loop (MT = 0)."""
    TT, RUN = _tiles(M, mm, 1)
    assert RUN is None
    L = cf.num_samples(3 * TT + 1, M, mm, 1, DCT) + 4
    _case(dev, "%d m%d r1 generic %s" % (M, mm, name), M, 1, 2, 3, L, name, mm=mm, seed=80 + mm)


@pytest.mark.parametrize("name", PROTOS)
@pytest.mark.parametrize("dct", [0, 2])
@pytest.mark.parametrize("M,r", GEOMS)
def test_short_and_odd_recordings(dev, M, r, dct, name):
    """Recordings shorter than one tile's window span (every tile an edge tile, zero fill on both sides), lengths that are no
    multiple of D, L % 4 in {1, 2, 3} (no vector loads).  With dct = 2 a recording that ends inside the look-ahead has no frames."""
    TT, D = _tiles(M, 4, r)[0], M >> r
    SPAN = (TT - 1) * D + 4 * M
    seen = 0
    for L in (1, D - 1, D + 1, SPAN - 1, SPAN + 1, 9 * D + 2, 9 * D + 7):
        X, _ = _case(dev, "%d r%d dct%d L=%d %s" % (M, r, dct, L, name), M, r, 2, 3, L, name, dct=dct, seed=90 + dct,
                     factor=_degenerate_factor(M, 4, r) if L == 1 else cf.FACTOR)
        seen += X.shape[-1] > 0
    assert seen == (7 if dct == 0 else 4)


def _raw_analysis(fb, rows, nsamples, pitch, S, N, X, tc, i16):
    """btk_fb_analysis / _i16 through the C-ABI with the caller's own pointer and pitch."""
    import ctypes as C
    import torch
    from distant_speech_recognition_amd import engine as eng
    lib = eng._lib.lib()
    fn = lib.btk_fb_analysis_i16 if i16 else lib.btk_fb_analysis
    eng.check(fn(fb._h, C.c_void_p(rows.data_ptr()), nsamples, pitch, S, N, C.c_void_p(X.data_ptr()), X.stride(2), 0, tc, None))
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", PROTOS)
@pytest.mark.parametrize("M", [512, 256, 1024])
def test_rows_pitch_and_alignment(dev, M, name):
    """Rows L + 3 apart that start 4 bytes past a 16-byte boundary (the scalar load path, interior tiles and a ragged last tile), and the
    same samples in aligned rows (the vector path): the same bits, the filling of 12345 beyond nsamples never read as signal.  Float
    samples and, where the bank takes them, int16."""
    import torch
    r, S, N = 1, 2, 3
    fb = _bank(M, 4, r, name)
    TT = _tiles(M)[0]
    L = cf.num_samples(4 * TT + 2, M, 4, r, DCT) + 6
    K, T = M // 2 + 1, fb.num_frames(L)
    assert T == 4 * TT + 3
    pcm = _pcm(S, N, L, 91)
    refs = _refs(M, 4, r, DCT, name, pcm)
    for i16 in ((False, True) if fb.analysis_i16() else (False,)):
        dtype, host = (torch.int16, pcm.astype(np.int16)) if i16 else (torch.float32, pcm)
        off, pitch, pitch_a = (2 if i16 else 1), L + 3, (L + 3) // 4 * 4 + 4
        flat = torch.zeros(S * N * pitch + off + 64, dtype=dtype, device=dev)
        rows = flat[off: off + S * N * pitch].view(S, N, pitch)
        rows_a = torch.zeros(S * N * pitch_a, dtype=dtype, device=dev).view(S, N, pitch_a)
        for t in (rows, rows_a):
            t[..., :L] = torch.from_numpy(host).to(dev)
            t[..., L:] = 12345                                  # beyond nsamples: must not be read as signal
        assert flat.data_ptr() % 16 == 0 and rows.data_ptr() % 16 == 4 and pitch % 4 and rows_a.data_ptr() % 16 == 0 and pitch_a % 4 == 0
        Xu = torch.empty((S, K, N, T), dtype=torch.complex64, device=dev)
        Xa = torch.empty((S, K, N, T), dtype=torch.complex64, device=dev)
        _raw_analysis(fb, rows, L, pitch, S, N, Xu, T, i16)
        _raw_analysis(fb, rows_a, L, pitch_a, S, N, Xa, T, i16)
        assert _same_bits(Xu, Xa)
        _judge_all("%d r%d rows %s %s" % (M, r, "int16" if i16 else "float32", name), Xu.cpu().numpy(), refs)


def _padded(dev, shape):
    """_guarded with rows an odd number of frames apart, more than the frames written."""
    import torch
    tc = shape[-1]
    row = tc + 2 + (tc % 2 == 0)
    assert row % 2 == 1 and row > tc
    return _guarded(dev, shape, torch.complex64, row)


@pytest.mark.parametrize("name", PROTOS)
@pytest.mark.parametrize("M,r", GEOMS)
def test_frame_ranges_and_padded_output(dev, M, r, name):
    """[t0, t0 + tcount) written into a [..., :tcount] view of a row-padded buffer between guard bands: the slice of the whole launch bit
    for bit, within the rule on its own, and nothing written outside the view."""
    import torch
    TT, RUN = _tiles(M, 4, r)
    RUN = RUN or 3
    S, N, K = 2, 3, M // 2 + 1
    L = cf.num_samples(RUN * TT + TT + 4, M, 4, r, DCT)
    fb = _bank(M, 4, r, name)
    pcm = _pcm(S, N, L, 95)
    refs = _refs(M, 4, r, DCT, name, pcm)
    p = torch.from_numpy(pcm).to(dev)
    whole = fb.analysis(p)
    tag = "%d r%d ranges %s" % (M, r, name)
    worst = _judge_all(tag + " whole", whole.cpu().numpy(), refs, show=False)
    for t0 in (1, TT - 1, TT, RUN * TT - 1):
        for tc in (1, TT, TT + 5):
            out, check = _padded(dev, (S, K, N, tc))
            fb.analysis(p, t0=t0, tcount=tc, out=out)
            host = out.cpu().numpy()
            check()
            assert _same_bits(out, whole[..., t0:t0 + tc]), (t0, tc)
            fig = _judge_all("%s t0=%d tc=%d" % (tag, t0, tc), host, refs, t0=t0, show=False)
            worst = fig if fig["ratio"] > worst["ratio"] else worst
    print(cf.cfratio_line(tag, worst))


@pytest.mark.parametrize("name", PROTOS)
@pytest.mark.parametrize("M", [512, 1024, 64])
def test_bin_shards(dev, M, name):
    """A bin shard, a ragged last tile, t0 = 1 and padded output: rows k0 .. k1 of the closed form itself, not of another launch."""
    import torch
    r, S, N, K = 1, 2, 3, M // 2 + 1
    TT = _tiles(M)[0]
    t0, tc = 1, TT + 5
    L = cf.num_samples(t0 + tc + TT, M, 4, r, DCT)
    fb = _bank(M, 4, r, name)
    pcm = _pcm(S, N, L, 97)
    refs = _refs(M, 4, r, DCT, name, pcm)
    p = torch.from_numpy(pcm).to(dev)
    for k0, k1 in ((0, 1), (K - 1, K), (K // 3, K // 3 + 7), (K // 2, K)):
        out, check = _padded(dev, (S, k1 - k0, N, tc))
        fb.analysis(p, t0=t0, tcount=tc, out=out, bins=(k0, k1))
        host = out.cpu().numpy()
        check()
        _judge_all("%d r%d bins [%d, %d) %s" % (M, r, k0, k1, name), host, refs, t0=t0, bins=(k0, k1),
                   factor=_degenerate_factor(M) if k1 - k0 == 1 else cf.FACTOR)


@pytest.mark.parametrize("name", PROTOS)
@pytest.mark.parametrize("M", [512, 256, 1024, 2048])
def test_int16_entry(dev, M, name):
    """One case per route that has the int16 form: the float launch's bits, and within the rule itself."""
    if not _bank(M, 4, 1, name).analysis_i16():
        return
    TT = _tiles(M)[0]
    args = (M, 1, 2, 3, cf.num_samples(4 * TT + 1, M, 4, 1, DCT) + 2, name)
    Xf, refs = _case(dev, "%d r1 float32 entry %s" % (M, name), *args, seed=99)
    Xi, _ = _case(dev, "%d r1 int16 entry %s" % (M, name), *args, seed=99, i16=True, refs=refs)
    assert np.array_equal(Xf.view(np.uint32), Xi.view(np.uint32))


# ---- the kernels behind the switches (read once per process: one child each) ----------------------------------------------------
SETTINGS = [("BTK_DISABLE_ANALYSIS512", "BTK_DISABLE_SYNTHESIS512"), ("BTK_DISABLE_FAST",),
            ("BTK_DISABLE_ANALYSIS512", "BTK_DISABLE_SYNTHESIS512", "BTK_DISABLE_FAST"), ("BTK_SYN_NARROW",)]
SWITCH_M = (512, 256, 1024)


def _switch_cases(off):
    """The frames and the channels axis at M = 512, 256, 1024 with the tile sizes of the kernel that runs under the switches `off`."""
    out = []
    for M in SWITCH_M:
        TT, RUN = _tiles(M, 4, 1, off)
        out += [(M,) + c for c in _frames_cases(M, 1, TT, RUN) + _channels_cases(M, 1, TT)]
    return out


def _switch_syn_cases():
    return [(g, T) for g in syn.SYN_SWITCH_GEOMS for T in syn._syn_switch_frames(*g)]


def _child_main(setting, path):
    import torch
    dev = torch.device("cuda", 0)
    off = SETTINGS[int(setting)]
    assert all(os.environ.get(k) == "1" for k in off)
    out = {}
    for i, (M, tag, S, N, L, tcount, seed) in enumerate(_switch_cases(off)):
        fb = _bank(M, 4, 1, "dense")
        assert fb.analysis_i16() == (_route(M, 4, 1, off) != "GENERIC")
        out["a%d" % i] = fb.analysis(torch.from_numpy(_pcm(S, N, L, seed)).to(dev), tcount=tcount).cpu().numpy()
    for i, (g, T) in enumerate(_switch_syn_cases()):
        for j, (label, b0, c, host) in enumerate(syn._syn_launches(dev, *g, T, reduced=True)):
            out["s%d_%d" % (i, j)] = host
            out["s%d_%d_piece" % (i, j)] = np.array([b0, c])
    np.savez(path, **out)
    print("child ok: " + setting)


_CHILD = "import sys; sys.path.insert(0, sys.argv[1]); from tests import test_gpu_analysis_closed_form as t; t._child_main(sys.argv[2], sys.argv[3])"


def test_kernels_behind_the_switches(dev):
    """The fb_fast.hip kernel instantiated at M = 512, the generic kernel at M >= 256 with m = 4, and the narrow synthesis forms: each
    setting in a fresh process of its own, one after another, none started after a failure; the parent judges what they saved."""
    base = {k: v for k, v in os.environ.items() if k not in BTK_SWITCHES}
    ref_cache = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, off in enumerate(SETTINGS):
            path = os.path.join(tmp, "setting_%d.npz" % i)
            res = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(i), path], env={**base, **{k: "1" for k in off}},
                                 capture_output=True, text=True, timeout=240, cwd=ROOT)
            assert res.returncode == 0 and "child ok: %d" % i in res.stdout, (off, res.returncode, res.stdout[-1500:], res.stderr[-2500:])
            with np.load(path) as z:
                got = {k: z[k] for k in z.files}
            os.remove(path)
            what = "+".join(k[4:] for k in off)
            for j, (M, tag, S, N, L, tcount, seed) in enumerate(_switch_cases(off)):
                key = (M, S, N, L, seed)
                if key not in ref_cache:
                    ref_cache[key] = _refs(M, 4, 1, DCT, "dense", _pcm(S, N, L, seed))
                X = got["a%d" % j]
                assert X.shape == (S, M // 2 + 1, N, cf.num_frames(L, M, 4, 1, DCT) if tcount is None else tcount)
                _judge_all("%s: %d r1 %s" % (what, M, tag), X, ref_cache[key])
            for j, (g, T) in enumerate(_switch_syn_cases()):
                pieces = syn._syn_pieces(T - cf.fb_delays(g[1], g[2], True, g[3])[0], reduced=True)
                launches = []
                for q, (kind, (b0, c)) in enumerate([(kind, pc) for kind in ("contiguous", "odd stride") for pc in pieces]):
                    assert tuple(got["s%d_%d_piece" % (j, q)]) == (b0, c)
                    launches.append(("%s b0=%d bc=%d" % (kind, b0, c), b0, c, got["s%d_%d" % (j, q)]))
                syn._syn_judge("%s: %s" % (what, syn._syn_tag(*g, T)), *g, T, launches)
