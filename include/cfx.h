/*
 * cfx.h - C-ABI of libcfx.so: MI355X (gfx950) residual-compressed activation exchange kernels.
 *
 * This is the drop-in boundary for CompactFusion's compressor hot path.  The reference has no
 * FFI (it is Python + Triton); these entry points are what a binding for that
 * path would call, one per reference kernel wrapper:
 *
 *   cfx_compress[_batch]   replaces  binary_quant_fastpath   xfuser/compact/fastpath.py:124-228  (+ eager scale prologue :150-166)
 *                                    int2_quant_fastpath     xfuser/compact/fastpath.py:584-669  (+ prologue :614-625)
 *                                    quantize_int8 on delta  xfuser/compact/compress_quantize.py:428-471 composed with main.py:227-233
 *                                    quantize_int4 on delta  xfuser/compact/compress_quantize.py:522-583 composed with main.py:227-233
 *                                    topk_compress           xfuser/compact/compress_topk.py:11-105 (slowpath.py:76-79)
 *                                    and the wire packing    xfuser/compact/main.py:149-152, slowpath.py:83
 *   cfx_decompress[_batch] replaces  binary_dequant_fastpath xfuser/compact/fastpath.py:371-438
 *                                    int2_dequant_fastpath   xfuser/compact/fastpath.py:745-811
 *                                    dequantize_int8/int4    xfuser/compact/compress_quantize.py:473-484, :585-640 (+ base add main.py:376)
 *                                    topk_decompress         xfuser/compact/compress_topk.py:108-163
 *                                    and the wire unpacking  xfuser/compact/main.py:285-304, slowpath.py:137-169
 *   cfx_packet_bytes       replaces  the size arithmetic of  xfuser/compact/main.py:285-293, slowpath.py:111-135
 *
 * Conventions
 *   - All tensor pointers are DEVICE pointers to contiguous row-major (N, C) fp16 ("half") data - or, for the 1-bit and 2-bit
 *     codecs, bf16 data: see "bf16 activations" below.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls are asynchronous.
 *   - No torch types, no exceptions: every call returns CFX_OK (0) or a negative error code and
 *     records a message retrievable with cfx_last_error_string().
 *   - The library keeps no state besides the opaque cfx_ctx (device id, tuning, last error).
 *     Workspace is caller-provided so calls can be captured in a hipGraph.
 *
 * Wire layouts (little endian; identical to the reference where the reference defines one)
 *   BINARY  [ bits  N*C/8 B : bit i of byte j of row n = (x-base)[n,8j+i] >= 0 | U  N fp16 | V  C fp16 ]   main.py:149-152
 *   INT2    [ codes N*C/4 B : 2-bit (sign<<1|mag) , element j at bits 2(j%4)   | tok N fp16 | chan C fp16 ]   main.py:149-152
 *   INT4    [ codes N*C/2 B : byte [n/2][c] = q[n][c] | q[n+1][c]<<4           | scale C fp16 | min C fp16 ]   compress_quantize.py:566-573
 *   INT8    [ q     N*C   B : int8                                             | scale C fp16 | zp  C int16 ]  compress_quantize.py:463-471
 *   INT2_MINMAX [ codes N*C/4 B : byte [n/4][c] = q[n][c] | q[n+1][c]<<2 | q[n+2][c]<<4 | q[n+3][c]<<6 | scale C fp16 | min C fp16 ]
 *           (no wire in the reference, which only simulates it: compress_quantize.py:386-426; INT4's row-per-byte convention, four rows)
 *   TOPK    [ val N*C/m fp16 | idx N*C/(2m) B : (i1<<4)|i2 per 2m-block of the flat (-1,1024) view ]           slowpath.py:76-79
 *   MXFP4   [ codes N*C/2 B : byte [n][j] = code[n][2j] | code[n][2j+1] << 4 | scale N*C/32 B : one E8M0 byte per block, row-major ]
 *           (no wire in the reference: the OCP Microscaling format, blocks of 32 consecutive elements of a row)
 *   BINARY_BLOCK [ bits N*C/8 B : bit i of byte j of row n = d[n,8j+i] >= 0 (BINARY's bit layout) | scale N*C/B fp16 : row-major, one per block ]
 *           (no wire in the reference: the block-wise sign compressor of 1-bit Adam / block signSGD, B = param consecutive elements of a row)
 *   INT2_BLOCK [ codes N*C/4 B : INT2's code layout, element j of a row at bits 2(j%4) of byte j/4 | scale N*C/B fp16 : row-major, one per block ]
 *           (no wire in the reference: INT2's sign / magnitude levels around BINARY_BLOCK's block scale)
 *   INT3_BLOCK [ hi N*C/4 B : 2-bit (sign<<1 | mag>>1), INT2's code layout | lo N*C/8 B : bit = mag & 1, BINARY's bit layout | scale N*C/B fp16 : row-major, one per block ]
 *           (no wire in the reference: a sign and four magnitude levels around BINARY_BLOCK's block scale)
 *   MXINT8  [ codes N*C B : element j of the flat view at byte j, two's complement | scale N*C/32 B : one E8M0 byte per block, row-major ]
 *           (no wire in the reference: the OCP Microscaling format, blocks of 32 consecutive elements of a row)
 *   The sections after the first start at the byte offsets these sizes give: they need not be 16-byte aligned (int8 with C % 16 == 8
 *   and N odd, int4 with C % 16 == 8 and N/2 odd, INT2_MINMAX with C % 16 == 8 and N/4 odd, 1-bit / 2-bit whenever N*C/8 resp. N*C/4 is not a multiple of 16).
 *   INT4 `min` of a channel whose minimum is zero: where zeros of BOTH signs occur among the channel's deltas, `min` may hold either zero
 *   (+0 or -0: a min reduction keeps the zero it meets first, and the order is the launch form's - waves, then row tiles).  Scale, codes,
 *   reconstruction and error-feedback state do not depend on it: q * scale >= +0, and (+0) + (-0) = +0.  Every other half of every packet
 *   is a function of the inputs alone.
 *
 * INT2_MINMAX (CFX_CODEC_INT2_MINMAX, param 0): INT4's arithmetic with 4 levels, one fp16 rounding per reference operation
 *       d      = x - base                                   (base NULL: x)
 *       mn, mx = per-channel min / max of d over the rows   (NaN-propagating, as int4 / int8)
 *       scale  = fp16( fp32(fp16(mx - mn)) / 3.000001f )
 *       q      = clamp( rint( fp16( fp16(d - mn) / scale ) ), 0, 3 )     round half to even; a NaN quotient gives code 0
 *       recv   = fp16( fp16(q * scale) + mn )
 *       new_base = base + recv     (CFX_FLAG_NO_EF: x)
 *   Shapes: C % 8 == 0 and N % 4 == 0 (CFX_ERR_SHAPE otherwise); cfx_packet_bytes = N*C/4 + 4*C; the workspace is INT4's.  The
 *   signed-zero rule for `min` and the non-finite rules are INT4's (above / "Non-finite input").  On a channel whose deltas are all equal
 *   the scale is 0 and the quotient NaN: the wire codec stores code 0 and reconstructs `min`, as INT4 does, where the reference's
 *   sim_int2_minmax returns NaN; everywhere else recv equals sim_int2_minmax(d) bit for bit.  Every launch form INT4 has exists
 *   (stand-alone, in-launch finalize, the one-launch layer with its gated / exchange forms); the quantise / dequantise kernels report
 *   INT4's kernel ids (cfx_profile_enable).  Ride-along reconstruction items (cfx_compress_batch_ex, n_ride > 0) stay the 1-bit codec's:
 *   with codec 6, as with INT4, they are CFX_ERR_CODEC.
 *
 * MXFP4 (CFX_CODEC_MXFP4 = 8, param 0; any other param: CFX_ERR_SHAPE, sizes 0): the OCP Microscaling (MX v1.0) conversion - floor
 *   scale, round-to-nearest-even elements, saturation - with a lower clamp on the shared exponent so that decode never leaves fp16.
 *   Blocks are 32 consecutive elements of a row (C % 32 == 0: also blocks of the flat view, never straddling rows); a block's scale is
 *   a function of that block alone, so the codec is one streaming pass with nothing global to wait for.  Bit for bit, one fp16 rounding
 *   per line:
 *       d      = fp16(x - base)                                   (base NULL: x)
 *       a      = max over the block of (bits(d) & 0x7fff)         (integer max: the largest magnitude)
 *       a >= 0x7c00 (a NaN or an inf in the block): scale byte 0xFF, all 16 code bytes 0, every element of the block reconstructs to a NaN
 *       e      = max( floor(log2 |d|max), -21 )                   (normal: (a >> 10) - 15; subnormal: from the leading bit; a == 0 gives -21)
 *       X      = e - 2            scale byte = X + 127            (so X in [-23, 13], bytes 104 ... 140)
 *       y      = |d| / 2^X                                         (exact; y < 8 by construction)
 *       mag    = index of the grid point {0, 0.5, 1, 1.5, 2, 3, 4, 6} nearest to y; a tie goes to the EVEN index; y > 6 saturates to index 7
 *       code   = (sign bit of d) << 3 | mag                        (a negative delta that rounds to magnitude 0 keeps its sign bit: code 8)
 *       recv   = (+-) grid[mag] * 2^X                              (exactly representable in fp16: that is what the clamp at -21 buys; |recv| <= 49152)
 *       new_base = recon = fp16(base + recv)                       (base NULL: recv;  CFX_FLAG_NO_EF: new_base = x)
 *   Shapes: C % 64 == 0, any N >= 1 (the packet length is even and every section a whole number of 32-bit words); cfx_packet_bytes =
 *   N*C/2 + N*C/32 (4.25 bits per element); cfx_workspace_bytes is 0, as for top-k: callers pass NULL / 0.  Forms: stand-alone compress /
 *   decompress (they report top-k's kernel ids, 13 and 14) and the one-launch layer k_mx_layer (the gated layer id, 31), taken under
 *   k_topk_layer's conditions - gated items, cfx_set_gated_launch on, no capture, a stream of >= 128 CUs, loop-back items reading this
 *   launch's packets; otherwise, and under stream capture, compress ; (exchange) ; decompress in stream order with the same results.
 *   Refused, as for INT4: CFX_ELEM_BF16 (CFX_ERR_CODEC, sizes 0), the second-order entry points and cfx_plan_set_second_order
 *   (CFX_ERR_CODEC: residual 2 composes cfx_residual2_delta / _update around the codec), ride-along items (CFX_ERR_CODEC).  Id 7 is no codec.
 *
 * BINARY_BLOCK (CFX_CODEC_BINARY_BLOCK = 10, param = the block size B in {32, 64, 128}; any other param: CFX_ERR_SHAPE, sizes 0): sign
 *   bits plus one fp16 abs-mean per block of B consecutive elements of a row.  A block's scale is a function of that block alone, so -
 *   unlike BINARY's rank-1 scales - the codec is one streaming pass with nothing global to wait for.  Bit for bit:
 *       d        = fp16(x - base)                                 (base NULL: x)
 *       bit      = d >= 0                                         (-0 gives 1; a NaN would give 0)
 *       s        = fp16( fp32(exact sum of |d| over the block, in units of 2^-24) / fp32(B) )
 *                  (mean16 of the sum of habs_units, cfx_device.h; mean16_exact of oracle/ref_np.py; the sum is exact: order-independent)
 *       recv     = bit ? s : -s                                   (s == 0: +0 / -0; |recv| <= 65504 always: a mean never exceeds its maximum)
 *       new_base = recon = fp16(base + recv)                      (base NULL: recv, bits verbatim;  CFX_FLAG_NO_EF: new_base = x)
 *   Shapes: C % max(B, 64) == 0, any N >= 1 (blocks never straddle rows, the bit section is a whole number of 64-bit words, the packet
 *   has an even number of halves); cfx_packet_bytes = N*C/8 + 2*N*C/B (1.5 / 1.25 / 1.125 bits per element); cfx_workspace_bytes is 0, as
 *   for top-k and MXFP4: callers pass NULL / 0.  CFX_ELEM_BF16 is accepted (codec argument 0x10A) under the "bf16 activations" rules below.
 *   Forms: stand-alone compress / decompress (they report top-k's kernel ids, 13 and 14) and the one-launch layer k_bb_layer (the gated
 *   layer id, 31), taken under k_mx_layer's conditions - gated items, cfx_set_gated_launch on, no capture, a stream of >= 128 CUs,
 *   loop-back items reading this launch's packets; otherwise, and under stream capture, compress ; (exchange) ; decompress in stream
 *   order with the same results.  Refused, as for MXFP4: the second-order entry points and cfx_plan_set_second_order (CFX_ERR_CODEC:
 *   residual 2 composes cfx_residual2_delta / _update around the codec), ride-along items (CFX_ERR_CODEC), any other high bit on the
 *   codec argument (CFX_ERR_CODEC, sizes 0).  Id 9 is no codec.
 *
 * INT2_BLOCK (CFX_CODEC_INT2_BLOCK = 12, param = the block size B in {32, 64, 128}; any other param: CFX_ERR_SHAPE, sizes 0): INT2's
 *   sign / magnitude codes and levels with the threshold taken as BINARY_BLOCK's scale - the abs-mean of the block of B consecutive
 *   elements of a row the element lies in.  Nothing global to wait for, as for BINARY_BLOCK.  Bit for bit, one fp16 rounding per line:
 *       d        = fp16(x - base)                                 (base NULL: x)
 *       s        = fp16( fp32(exact sum of |d| over the block, in units of 2^-24) / fp32(B) )         (BINARY_BLOCK's scale)
 *       sign     = d >= 0                                         (-0 gives 1)
 *       mag      = |d| > s                                        (strict; compared as fp16 values = their magnitude bits as integers)
 *       code     = sign << 1 | mag                                (INT2's code)
 *       small    = fp16(0.5 * s)                                  (round to nearest even: matters only for subnormal s; s = 2^-24 gives 0)
 *       large    = fp16( min( 2 * fp32(s), 65504 ) )              (saturating, never inf: INT2 leaves that overflow unspecified)
 *       recv     = (sign ? + : -) (mag ? large : small)           (s == 0: +0 / -0 by the sign bit)
 *       new_base = recon = fp16(base + recv)                      (base NULL: recv, bits verbatim;  CFX_FLAG_NO_EF: new_base = x)
 *   Shapes are BINARY_BLOCK's: C % max(B, 64) == 0, any N >= 1; cfx_packet_bytes = N*C/4 + 2*N*C/B (2.5 / 2.25 / 2.125 bits per
 *   element); cfx_workspace_bytes is 0: callers pass NULL / 0.  CFX_ELEM_BF16 is accepted (codec argument 0x10C) under the "bf16
 *   activations" rules below.  Forms and fall-backs are BINARY_BLOCK's: stand-alone compress / decompress (kernel ids 13 and 14) and the
 *   one-launch layer k_i2b_layer (id 31) under k_bb_layer's conditions; otherwise, and under stream capture, compress ; (exchange) ;
 *   decompress in stream order with the same results.  Refused, as for BINARY_BLOCK: the second-order entry points and
 *   cfx_plan_set_second_order (CFX_ERR_CODEC: residual 2 composes cfx_residual2_delta / _update around the codec), ride-along items
 *   (CFX_ERR_CODEC), any other high bit on the codec argument (CFX_ERR_CODEC, sizes 0).  Id 11 is no codec.
 *
 * INT3_BLOCK (CFX_CODEC_INT3_BLOCK = 14, param = the block size B in {32, 64, 128}; any other param: CFX_ERR_SHAPE, sizes 0): a sign and
 *   one of four magnitude levels, thresholds and levels taken from BINARY_BLOCK's scale - the abs-mean of the block of B consecutive
 *   elements of a row the element lies in.  Nothing global to wait for, as for BINARY_BLOCK.  Bit for bit, one rounding per line:
 *       d        = fp16(x - base)                                 (base NULL: x)
 *       s        = fp16( fp32(exact sum of |d| over the block, in units of 2^-24) / fp32(B) )         (BINARY_BLOCK's scale)
 *       t_k      = fp16( min( fp32(s) * T_k, 65504 ) )            T = {0.75, 1.5, 2.625}   (products exact in fp32; round to nearest even
 *                                                                 to fp16, subnormals included)
 *       l_k      = fp16( min( fp32(s) * L_k, 65504 ) )            L = {0.375, 1.125, 1.875, 3.375}   (saturating: never inf into a state)
 *       sign     = d >= 0                                         (-0 gives 1, as INT2_BLOCK)
 *       mag      = (|d| > t_0) + (|d| > t_1) + (|d| > t_2)        (strict; compared as fp16 values = their magnitude bits as integers; 0..3)
 *       recv     = (sign ? + : -) l_mag                           (s == 0: +0 / -0 by the sign bit)
 *       new_base = recon = fp16(base + recv)                      (base NULL: recv, bits verbatim;  CFX_FLAG_NO_EF: new_base = x)
 *   T and L: between the Lloyd-Max grids of a Gaussian and a Laplacian source of unit abs-mean, in eighths.  A scale past 65504 / 3.375
 *   saturates l_3; past 65504 / 2.625 and 65504 / 1.5 a threshold is 65504 and mag 3, then 2, is unreachable.  s = 2^-24 gives t = 1, 2, 3
 *   units and l_0 = 0.  Wire: three sections, no padding -
 *       hi    N*C/4 bytes   2-bit (sign << 1 | mag >> 1), INT2's code layout: element j of a row at bits 2(j%4) of byte j/4
 *       lo    N*C/8 bytes   bit = mag & 1, BINARY's bit layout: bit i of byte j of row n = element 8j+i
 *       scale 2*N*C/B bytes fp16, row-major, one per block
 *   Shapes are BINARY_BLOCK's: C % max(B, 64) == 0, any N >= 1; cfx_packet_bytes = 3*N*C/8 + 2*N*C/B (3.5 / 3.25 / 3.125 bits per
 *   element); cfx_workspace_bytes is 0: callers pass NULL / 0.  CFX_ELEM_BF16 is accepted (codec argument 0x10E) under the "bf16
 *   activations" rules below.  Forms and fall-backs are INT2_BLOCK's: stand-alone compress / decompress (kernel ids 13 and 14) and the
 *   one-launch layer k_i3b_layer (id 31) under k_i2b_layer's conditions; otherwise, and under stream capture, compress ; (exchange) ;
 *   decompress in stream order with the same results.  Refused, as for INT2_BLOCK: the second-order entry points and
 *   cfx_plan_set_second_order (CFX_ERR_CODEC: residual 2 composes cfx_residual2_delta / _update around the codec), ride-along items
 *   (CFX_ERR_CODEC), any other high bit on the codec argument (CFX_ERR_CODEC, sizes 0).  Ids 13 and 15 are no codecs (17 is none).
 *
 * MXINT8 (CFX_CODEC_MXINT8 = 16, param 0; any other param: CFX_ERR_SHAPE, sizes 0): the OCP Microscaling (MX v1.0) INT8 element - an
 *   int8 with an implied 2^-6 - under one E8M0 power-of-two scale per 32 consecutive elements of a row (C % 32 == 0: also blocks of the
 *   flat view), with MXFP4's floor scale and a lower clamp on the shared exponent so that decode never leaves fp16.  A block's scale is
 *   a function of that block alone: one streaming pass, no statistic to wait for, no workspace.  Bit for bit, one rounding per line:
 *       d      = fp16(x - base)                                   (base NULL: x;  bf16: "bf16 activations" below)
 *       a      = max over the block of (bits(d) & 0x7fff)         (integer max: the largest magnitude)
 *       a >= 0x7c00 (a NaN or an inf in the block): scale byte 0xFF, all 32 code bytes 0, every element of the block reconstructs to NaN (0x7e00)
 *       e      = floor(log2 |d|max)                               (normal: (a >> 10) - 15; subnormal: from the leading bit; a == 0: below the clamp)
 *       X      = max(e, -18)      scale byte = X + 127            (so X in [-18, 15], bytes 109 ... 142)
 *       y      = d * 2^(6 - X)                                    (exact in fp32: an 11-bit significand times a power of two; |y| < 128)
 *       q      = clamp( round-to-nearest-even(y), -127, 127 )     (symmetric: -128 is never sent)
 *       code   = q as a two's-complement byte                     (a -0 or a negative delta that rounds to 0 sends 0x00)
 *       recv   = q * 2^(X - 6)                                    (exact in fp16: |q| <= 127 times a power of two >= 2^-24 - what the clamp at -18
 *                                                                 buys; |recv| <= 65024; q == 0 gives +0, bits 0x0000)
 *       new_base = recon = fp16(base + recv)                      (base NULL: recv, bits verbatim;  CFX_FLAG_NO_EF: new_base = x)
 *   So |d - recv| <= 2^(X-7) wherever |y| <= 127.5 and <= (15/16) 2^(X-6) otherwise (saturation: only the top 1/128 of a binade), and a
 *   block with |d|max < 2^-17 is reproduced exactly.  A receiver reads the byte 0x80 as -127; a scale byte outside 109 ... 142 other than
 *   0xFF is never sent and its result is unspecified.  Wire: two sections, no padding -
 *       codes N*C bytes     element j of the flat view at byte j
 *       scale N*C/32 bytes  block k at byte N*C + k
 *   Shapes: C % 64 == 0, any N >= 1; cfx_packet_bytes = N*C + N*C/32 (8.25 bits per element); cfx_workspace_bytes is 0: callers pass
 *   NULL / 0.  CFX_ELEM_BF16 is accepted (codec argument 0x110) under the "bf16 activations" rules below.  Forms: stand-alone compress /
 *   decompress (they report top-k's kernel ids, 13 and 14) and the one-launch layer k_mxi8_layer (the gated layer id, 31), taken under
 *   k_mx_layer's conditions; otherwise, and under stream capture, compress ; (exchange) ; decompress in stream order with the same
 *   results.  Refused, as for the other block-local codecs: the second-order entry points and cfx_plan_set_second_order (CFX_ERR_CODEC:
 *   residual 2 composes cfx_residual2_delta / _update around the codec), ride-along items (CFX_ERR_CODEC), any other high bit on the
 *   codec argument (CFX_ERR_CODEC, sizes 0).
 *
 * bf16 activations (CFX_CODEC_BINARY, CFX_CODEC_INT2, CFX_CODEC_BINARY_BLOCK, CFX_CODEC_INT2_BLOCK, CFX_CODEC_INT3_BLOCK and CFX_CODEC_MXINT8 only)
 *   CFX_ELEM_BF16 or-ed into the `codec` argument of an entry point that takes one (cfx_packet_bytes, cfx_workspace_bytes,
 *   cfx_compress[_batch[_ex|_gated]], cfx_decompress[_batch], cfx_plan_add_compress[_ex|_gated], cfx_plan_add_decompress,
 *   cfx_plan_add_exchange_layer[_p2p], and through them cfx_plan_copy_op) says that ALL tensor operands of the call - x, base, new_base,
 *   recon, of the compress, ride-along and gated items alike - are bf16.  cfx_int2_quantize, which has no codec argument, takes
 *   CFX_FLAG_ELEM_BF16 in `flags`.  The residual domain and the wire stay fp16:
 *       d        = fp16_rne( fp32(x) - fp32(base) )          one fp32 subtraction, one rounding to fp16; base NULL: d = fp16_rne(fp32(x))
 *       d -> recv  exactly the fp16 path: sign bits / 2-bit codes, exact sums in units of 2^-24, fp16 scales, packet bytes;
 *                  recv = (2b - 1) * fp16(u * v)  or the 2-bit levels  or +-s of the block (BINARY_BLOCK)  or the block's two / four levels (INT2_BLOCK / INT3_BLOCK)  or q * 2^(X-6) (MXINT8), in fp16
 *       new_base = recon = bf16_rne( fp32(base) + fp32(recv) )     base NULL: bf16_rne(fp32(recv))
 *       CFX_FLAG_NO_EF: new_base = x, copied verbatim as bf16 bits
 *   Packet layout, cfx_packet_bytes and cfx_workspace_bytes are those of the fp16 codec: a bf16 sender's packet is a valid fp16-path
 *   packet (a receiver may reconstruct it onto an fp16 state with the plain codec id, and the other way round).  Domain as for the
 *   fp16 path: finite inputs with |x - base| < 65504; outside it the result is unspecified (see "Non-finite input").
 *   The bit on codecs 3 - 6 and 8, and any other bit above the codec id, is CFX_ERR_CODEC; the sizes of such a codec argument are 0.
 *   Every form the fp16 path has exists for bf16 (stand-alone, in-launch finalize, ride-along, one-launch layer forms, the peer-to-peer
 *   exchange inside the launch), with the documented fall-backs; cfx_plan_run_pipelined and the rank-K 1-bit codec are fp16 only (a
 *   pipelined replay of bf16 ops runs as cfx_plan_run).
 *
 * Second-order residual (CFX_CODEC_BINARY and CFX_CODEC_INT2 only, fp16; CompactConfig(residual=2), xfuser/compact/main.py:244-266, :378-384)
 *   cfx_compress_batch_res2 / cfx_decompress_batch_res2 take, beside each item, a cfx_second_item {delta_base, new_delta_base} and the
 *   decay factor (CompactConfig.delta_decay_factor, main.py:272-273); cfx_plan_set_second_order attaches the same to a plan op.  The
 *   predictor is base + delta_base; one fp16 rounding per reference operation:
 *       dd        = fp16( fp16(x - base) - delta_base )                  what the codec sees (as if base were NULL)
 *       dd -> recv  exactly the fp16 codec: sign bits / 2-bit codes, exact sums in units of 2^-24, fp16 scales, packet bytes
 *       new_base  = recon = fp16( fp16(base + delta_base) + recv )
 *       new_delta = fp16( fp32( fp16(delta_base + recv) ) * fp32(decay) )
 *   The packet is a plain fp16-path packet of the same codec; cfx_packet_bytes and cfx_workspace_bytes are the codec's.  Results - packet
 *   bytes, new_base, new_delta - are bit for bit what cfx_residual2_delta ; cfx_compress_batch(base NULL) ; cfx_decompress_batch(base
 *   NULL) ; cfx_residual2_update produce, in one launch sequence of the codec's own (the second-order kernels read delta_base beside
 *   base in their tile loops and store both states where the first-order kernels store one; no full-size temporaries).
 *   In place is allowed: new_base == base, new_delta_base == delta_base.  base and delta_base are required (CFX_ERR_NULL); a
 *   reconstruction item may have new_delta_base NULL (update_cache = False: recon only); a compress item needs new_base and
 *   new_delta_base with CFX_FLAG_UPDATE_CACHE and writes only the packet without it.  CFX_ERR_CODEC before any launch: CFX_FLAG_NO_EF
 *   (main.py ignores error_feedback with residual 2), CFX_ELEM_BF16, codec ids 3 - 6, 8, 10, 12, 14 and 16 (those compose cfx_residual2_delta / _update
 *   around the codec).  The second-order launches report the kernel ids of their first-order twins (cfx_profile_enable).
 *
 * Non-finite input (NaN, +-inf in x or base, or an x - base that overflows or is inf - inf)
 *   INT4 / INT8 / INT2_MINMAX: the per-channel min and max propagate NaN as the reference's torch.min / torch.max do - a channel with a NaN delta gets
 *                a NaN scale (and min), codes 0, zero point 0 and a NaN reconstruction; +-inf flow through the fp16 arithmetic.
 *   TOPK:        |delta| is ranked as the reference's tl.argmax ranks it: NaN above everything, +inf included; the first NaN wins.
 *   MXFP4, MXINT8: a block with a NaN or an inf delta is the 0xFF block above (codes 0, NaN reconstruction); its neighbours are untouched.
 *   BINARY / INT2 / BINARY_BLOCK / INT2_BLOCK / INT3_BLOCK: unspecified.  Their scales are exact integer sums of |delta| (cfx_device.h habs_units), which cannot carry inf or
 *                NaN; the outputs are finite garbage or NaN, and need not match the reference.
 */
#ifndef CFX_H
#define CFX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CFX_ABI_VERSION 2
#define CFX_MAX_BATCH 16

typedef struct cfx_ctx cfx_ctx;

enum cfx_status {
    CFX_OK = 0,
    CFX_ERR_NULL = -1,       /* a required pointer is NULL */
    CFX_ERR_SHAPE = -2,      /* N/C/param violate the codec's divisibility rules */
    CFX_ERR_ALIGN = -3,      /* a tensor or packet pointer is not 16-byte aligned */
    CFX_ERR_CODEC = -4,      /* unknown codec id */
    CFX_ERR_BATCH = -5,      /* batch < 1 or > CFX_MAX_BATCH */
    CFX_ERR_LAUNCH = -6,     /* hipGetLastError() after a launch was not hipSuccess */
    CFX_ERR_WORKSPACE = -7,  /* workspace NULL or smaller than cfx_workspace_bytes() */
    CFX_ERR_GATE = -8,       /* an in-launch gate / lane flag wait of an EARLIER launch on this context timed out (cfx_gate_errors) */
    CFX_ERR_QUEUES = -9      /* flag-ordered streams asked for, but the process did not give HIP's streams hardware queues of their own
                              * (GPU_MAX_HW_QUEUES unset: cfx_hw_queues_ok) */
};

enum cfx_codec {
    CFX_CODEC_BINARY = 1,    /* COMPACT_COMPRESS_TYPE.BINARY fastpath, comp_rank = -1 */
    CFX_CODEC_INT2 = 2,      /* COMPACT_COMPRESS_TYPE.INT2 fastpath */
    CFX_CODEC_INT4 = 3,      /* per-channel min/max 16 levels, rows paired per byte */
    CFX_CODEC_INT8 = 4,      /* per-channel affine int8, zero point int16 */
    CFX_CODEC_TOPK = 5,      /* COMPACT_COMPRESS_TYPE.SPARSE, param = m in {1,2,4,8,16} */
    CFX_CODEC_INT2_MINMAX = 6, /* COMPACT_COMPRESS_TYPE.INT2_MINMAX: per-channel min/max 4 levels, four rows per byte; param 0 */
    CFX_CODEC_MXFP4 = 8,     /* COMPACT_COMPRESS_TYPE.MXFP4: FP4 E2M1 elements, one E8M0 scale per 32 of a row; param 0 (7 is no codec) */
    CFX_CODEC_BINARY_BLOCK = 10, /* COMPACT_COMPRESS_TYPE.BINARY_BLOCK: sign bits, one fp16 abs-mean per param = 32 / 64 / 128 of a row (9 is no codec) */
    CFX_CODEC_INT2_BLOCK = 12, /* COMPACT_COMPRESS_TYPE.INT2_BLOCK: INT2's codes, one fp16 abs-mean per param = 32 / 64 / 128 of a row (11 is no codec) */
    CFX_CODEC_INT3_BLOCK = 14, /* COMPACT_COMPRESS_TYPE.INT3_BLOCK: sign + 2 magnitude bits, one fp16 abs-mean per param = 32 / 64 / 128 of a row (13 is no codec) */
    CFX_CODEC_MXINT8 = 16    /* COMPACT_COMPRESS_TYPE.MXINT8: int8 elements (implied 2^-6), one E8M0 scale per 32 of a row; param 0 (15 is no codec) */
};
/* or-ed into a `codec` argument: the call's tensors are bf16 (1-bit, 2-bit, block-scaled 1-bit / 2-bit / 3-bit codecs and MXINT8; "bf16 activations" above) */
#define CFX_ELEM_BF16 0x100

enum cfx_flags {
    CFX_FLAG_UPDATE_CACHE = 1, /* write new_base (compact_compress(update_cache=True)) */
    CFX_FLAG_NO_EF = 2,        /* error feedback off: new_base = x (main.py:233 `else x`) */
    CFX_FLAG_ELEM_BF16 = 0x100 /* cfx_int2_quantize only (it has no codec argument): x, base, new_base are bf16 */
};

/* One tensor of a compress batch.  base may be NULL (compress_residual == 0: the codec sees x itself);
 * new_base may alias base (in-place error-feedback update) and is ignored unless CFX_FLAG_UPDATE_CACHE. */
typedef struct cfx_comp_item {
    const void* x;        /* (N,C) fp16 (bf16 with CFX_ELEM_BF16: all three tensors), 16-byte aligned */
    const void* base;     /* (N,C) fp16, 16-byte aligned, or NULL */
    void*       new_base; /* (N,C) fp16, 16-byte aligned, or NULL */
    void*       packet;   /* cfx_packet_bytes() bytes, 16-byte aligned */
} cfx_comp_item;

/* One tensor of a decompress batch.  recon = base + decode(packet) (base NULL: recon = decode(packet)).
 * recon may alias base (the receiver's cache update, main.py:317-319). */
typedef struct cfx_decomp_item {
    const void* packet;
    const void* base;
    void*       recon;
} cfx_decomp_item;

int         cfx_abi_version(void);
cfx_ctx*    cfx_create(int device);
void        cfx_destroy(cfx_ctx* ctx);
const char* cfx_last_error_string(cfx_ctx* ctx);

/* rows per workgroup tile for the streaming kernels (0 = automatic). */
int         cfx_set_rows_per_tile(cfx_ctx* ctx, int rows);

/* Size in bytes of one packet / of the scratch workspace a compress batch needs. 0 on invalid arguments. */
size_t      cfx_packet_bytes(int codec, int N, int C, int param);
size_t      cfx_workspace_bytes(int codec, int N, int C, int param, int batch);

int cfx_compress_batch(cfx_ctx* ctx, int codec, int N, int C, int param, int flags,
                       int batch, const cfx_comp_item* items,
                       void* workspace, size_t workspace_bytes, void* stream);

int cfx_decompress_batch(cfx_ctx* ctx, int codec, int N, int C, int param,
                         int batch, const cfx_decomp_item* items, void* stream);

/* cfx_compress_batch plus `n_ride` reconstruction items of the SAME codec and shape (1-bit codec only) that are
 * co-scheduled in the statistics launch: bandwidth work that does not depend on this call's scales - typically the previous
 * layer's deferred error-feedback update (own packet applied to own state; the reference does it inside
 * _binary_quant_fastpath, fastpath.py:88-120, but nothing reads that state before the next denoise step: the local
 * attention block uses the uncompressed K,V, ring.py:207-209) - streams while the scale reduction, which is pure
 * latency, completes.  The ride items must not alias this call's x / base / packet operands. */
int cfx_compress_batch_ex(cfx_ctx* ctx, int codec, int N, int C, int param, int flags,
                          int batch, const cfx_comp_item* items, int n_ride, const cfx_decomp_item* ride,
                          void* workspace, size_t workspace_bytes, void* stream);

/* cfx_compress_batch_ex plus `n_gated` reconstruction items (any streaming codec, same shape) whose PACKETS ARE PRODUCED BY THIS CALL:
 * typically the call's own packets applied to the rank's own state (the error-feedback update, fastpath.py:88-120) and -
 * when logical peers are looped back on one GPU - to the peers' states.  They run in the SAME launch as the compress: their
 * workgroups first pull the state tiles into registers (bandwidth work that overlaps the scale reduction, which is pure
 * latency), wait on an arrival counter until the packet is complete, then finish from registers.  One launch per layer instead
 * of two, 2.125 instead of 4.125 B/el behind the dependency.  With CFX_FLAG_UPDATE_CACHE the call's own error-feedback update
 * (new_base) is part of the launch too (1-bit: as two more gated tensors; 2-bit: the statistics workgroups quantise their own
 * tiles from registers once the scales exist, a second gate releases the gated items; int4 / int8: k_minmax_layer, the statistics tile kept
 * in registers, codes and the state update from them; top-k: k_topk_layer, nothing global to wait for - the gate counts the compress
 * workgroups).  Results are identical to compress
 * followed by cfx_decompress_batch; when the shape does not qualify (C % 128 != 0, statistics tile != 32 rows, in-launch
 * finalize off, too many items for one launch) exactly that sequence runs.
 * A gated item's base/recon must not alias this call's x / packet operands; recon may equal base, and a gated item may
 * update a compress item's `base` in place (the compress group has finished reading it when the gate opens).
 * Inside the launch (round 5): the 1-bit / 2-bit statistics tiles hand their partial sums over as TAGGED 8-byte words {24-bit launch
 * tag | 40-bit sum} in an arena the context keeps per stream (zeroed at allocation, tags never reused) - the data is its own "published"
 * mark: no drain, no ticket, and no 32-bit cliff (round 4's words gave out at an average |residual| of 0.5; beyond 40 bits - an average
 * of 128 - the exact sum travels in the caller's workspace); FIXED workgroups (the last-dispatched tiles) poll the words they reduce and
 * publish the scales into the packet and, tagged, into the arena.  2-bit: a statistics tile polls those tagged scales (no gate 1), and a
 * reconstruction tile waits for the 4 - 6 tiles whose codes it reads (per-tile flags) instead of the slowest of all (2.10 -> 1.89 ms per
 * FLUX step).  1-bit: the reconstruction tiles keep the arrival gate (XCD-relayed; tagged scales measured 10 % slower there).
 * Stream capture (round 6): the ONE-launch forms take the value their gates open at, their ticket-ring slot and their launch tags as launch
 * arguments the host advances with every launch (monotonic arrival counters, no reset, no memset node) - a replayed node would wait for
 * numbers that have gone by.  So on a CAPTURING stream this call - and the exchange-layer ops of a plan - enqueue the capturable sequence
 * instead: compress (tickets that reset themselves) ; reconstruct the gated items in stream order; identical results, two launches (int4 /
 * int8: three) instead of one, no host call per replay.  tests/test_gpu_api.py::test_layer_calls_are_graph_capturable replays every codec's
 * layer call and the peer-to-peer layer op four times between eager launches of the same context.  The ungated launches (cfx_compress_batch
 * / _ex) are capturable as they are.  (An int4 / int8 compress call outside a capture runs as ONE launch too - statistics, scales, codes
 * and the state update from the tile in registers, k_minmax_layer - handing its partials over as sequence-tagged words in an arena the
 * context keeps per stream; under stream capture the same call runs the capturable sequence statistics ; quantise, with identical results.)
 * ONE launch under capture (cfx_set_captured_layer below, off by default): the BLOCK-LOCAL codecs - top-k, MXFP4, BINARY_BLOCK, INT2_BLOCK,
 * INT3_BLOCK, MXINT8 - wait for nothing but "packets complete" (and the external gate), so their layer launch can derive its number on
 * the device: each captured layer call takes a private gate slot from a pool of the context, group S's arrivals and an entry ticket per
 * group-D workgroup are 64-bit fetch-adds on counters of that slot that only ever grow, launch number = counter / workgroups per launch,
 * and the gate opens at number + 1 - nothing is advanced or reset by anybody (csrc/cfx_capture_gate.h, csrc/cfx_capture.hip: separate
 * kernel instantiations, same bits; no eager launch changed).  The abs-mean and min/max layer launches (codecs 1 - 4, 6) carry
 * host-advanced launch tags in their hand-over words and always take the sequence under capture. */
int cfx_compress_batch_gated(cfx_ctx* ctx, int codec, int N, int C, int param, int flags,
                             int batch, const cfx_comp_item* items, int n_ride, const cfx_decomp_item* ride,
                             int n_gated, const cfx_decomp_item* gated,
                             void* workspace, size_t workspace_bytes, void* stream);
/* Number of in-launch gate / lane flag waits that timed out since the last call (a bounded spin gives up instead of hanging the GPU;
 * always 0 unless the library is broken or a stream was starved), or < 0 on error.  Reads and clears a pinned host word: no device
 * synchronisation (a complete count needs the streams drained first).  While the count is non-zero every compress / plan / merge
 * call on the context returns CFX_ERR_GATE. */
int cfx_gate_errors(cfx_ctx* ctx);
/* Every in-launch wait (arrival gates, tagged-word and flag polls, the peer-to-peer exchange inside a layer launch, the low-rank
 * hand-overs) gives up on ONE time base: the 100 MHz wall clock against the context's gate timeout (default 5 s,
 * cfx_set_gate_timeout_ms), never on an iteration count.  A workgroup whose wait gave up does NOT store: reconstructions from packets
 * that have not arrived are never written, the states the workgroup owns stay as they were, and the error word counts the failure.
 * The launch it belonged to leaves the context's arrival counters short; cfx_gate_recover drains the device, resets them (and the
 * low-rank hand-over arenas) and clears the error word, after which the context is usable again.  Returns the number of failed waits
 * that were pending, or < 0.  What the caller does about the layer whose exchange failed (run it again over another transport, or drop
 * the generation) is its business: compact/xlayer.py re-validates. */
int cfx_gate_recover(cfx_ctx* ctx);

/* The statistics pass of a compress call reduces its partial sums INSIDE the launch (last-arriving workgroups, ticket
 * counters; replaces the eager scale prologue of fastpath.py:150-166 / compress_quantize.py:452-463 and the separate
 * finalize kernel).  The tickets live in device memory owned by the context: cfx_prepare allocates them (idempotent;
 * otherwise the first compress call does - call it before capturing compress calls into a hipGraph).  Compress calls
 * on one context may come from several streams (a ticket ring per stream, 8 rings, the least recently used one is reassigned;
 * launches of one stream are in order).
 * cfx_set_fused_finalize(ctx, 0) selects the two-kernel sequence (statistics, finalize); results are bit-identical. */
int cfx_prepare(cfx_ctx* ctx);
int cfx_set_fused_finalize(cfx_ctx* ctx, int on);
/* (Developer probes - per-workgroup phase stamps, the launch-tag test hook, early exits of the compress kernel - are NOT part of this
 * library: include/cfx_dev.h, libcfx_dev.so, built with -DCFX_DEV_PROBES.) */
/* Tuning / measurement switches of a context.  The library reads NO environment variable for its behaviour (the one variable it looks
 * at, GPU_MAX_HW_QUEUES, belongs to the HIP runtime: see cfx_prepare below); what earlier builds read from the environment is set here:
 *   cfx_set_stats_rows    statistics tile height of the one-launch compress (multiple of 16; 0 = automatic)
 *   cfx_set_gated_launch  0: the gated / exchange-layer ops always run as compress ; exchange ; reconstruct in stream order (1 = default:
 *                         the one-launch forms where they qualify)
 *   cfx_set_lr_chain      low-rank factor chain: 0 = automatic (slab-resident single launch where its workgroups fit the stream, else
 *                         the six-launch N-space chain, else the C-space chain), 1 = never the single launch, 2 = C-space chain only
 *   cfx_set_lr_decode     low-rank reconstruction kernel: 0 = automatic (MFMA form at rank 32), 1 = VALU form, 2 = MFMA form.  The
 *                         sender's error-feedback update follows the switch: its state stays the receiver's reconstruction bit for bit */
int cfx_set_stats_rows(cfx_ctx* ctx, int rows);
int cfx_set_gated_launch(cfx_ctx* ctx, int on);
int cfx_set_lr_chain(cfx_ctx* ctx, int chain);
int cfx_set_lr_decode(cfx_ctx* ctx, int mode);
/* The block-local codecs' layer launch as ONE launch under hipGraph capture ("Stream capture" above).
 *   cfx_set_captured_layer(ctx, slots)   0 (default): a captured layer call enqueues the capturable sequence, as ever.  n in 1 .. 4096 (the
 *       maximum; 4224 bytes of device memory a slot): allocates and zeroes a pool of n private gate slots with their ticket lines - here,
 *       because nothing may be allocated during capture; call it outside a capture.  A negative value, one above 4096, or a CHANGE of the
 *       pool's size while slots are handed out is CFX_ERR_SHAPE (the same value again is CFX_OK and changes nothing).
 *   With a pool, a layer call on a CAPTURING stream takes a slot and enqueues the one capturable layer kernel when the codec is one of the
 *       six block-local families, the conditions of the eager one-launch form hold (gated items, cfx_set_gated_launch on, a stream of >= 128
 *       CUs, loop-back items that read this launch's packets - or the op is a peer-to-peer exchange-layer op, whose exchange runs inside the
 *       launch) and a slot is free: cfx_compress_batch_gated, and cfx_plan_run for cfx_plan_add_exchange_layer (no communicator) and
 *       cfx_plan_add_exchange_layer_p2p ops.  Every other case - no pool, no free slot, another codec, an exchange-layer op with a
 *       communicator - enqueues the capturable sequence with identical results.
 *   RULE: a slot belongs to ONE captured graph node, for as long as the graph may be replayed; every launch on a slot is that node, so the
 *       counters of the slot say which replay is running.  Replays of the graphs of one context must be stream-ordered against each other
 *       and against the context's other launches on the same buffers, as for workspaces.  Only loop-back items and world size 1 are covered
 *       under capture: with live peers the packet-slot parity and the group's health are host state a graph would bake in.
 *   cfx_captured_layer_stats   how many capture-time layer calls of the context took the one-launch form / the sequence (every codec's
 *       gated and exchange-layer calls count), and how many slots are free; any pointer may be NULL.
 *   cfx_captured_layer_release hands every slot back, zeroed, after a device synchronisation - for a caller that has DESTROYED its graphs
 *       (a surviving graph would share its slot with the next capture).
 *   cfx_gate_recover zeroes the pool as well: all-zero is "before launch 0", so live graphs stay valid.  A wait that gives up has drawn its
 *       ticket and group S always arrives, so a time-out leaves a slot consistent even without it. */
int cfx_set_captured_layer(cfx_ctx* ctx, int slots);
int cfx_captured_layer_stats(cfx_ctx* ctx, int* one_launch, int* sequence, int* slots_free);
int cfx_captured_layer_release(cfx_ctx* ctx);
/* Flag-ordered launches (the exchange-layer ops, the exchange lane) need the streams they order to sit on hardware queues of their own:
 * a polling kernel is never scheduled out for the kernel it waits for.  HIP multiplexes streams over a pool of hardware queues; with
 * GPU_MAX_HW_QUEUES unset a stream created after a collective library initialised can be time-sliced against the exchange stream's
 * queue (measured: the layer launch 25 -> 50-100 us, and gate time-outs under stream churn).  cfx_hw_queues_ok() returns 1 when the
 * process set the variable to >= 2 before HIP started (any explicit value restores one queue per stream), 0 otherwise.  With 0 the
 * plan ops that would order two streams by flags (cfx_plan_add_exchange_layer[_p2p] in their one-launch form, cfx_plan_run_lane) are
 * refused with CFX_ERR_QUEUES - the exchange-layer ops then run in stream order on one stream (same results) - unless
 * cfx_set_allow_shared_queues(ctx, 1) says the caller knows better. */
int cfx_hw_queues_ok(void);
int cfx_set_allow_shared_queues(cfx_ctx* ctx, int on);

/* Single-tensor conveniences (batch of one). */
int cfx_compress(cfx_ctx* ctx, int codec, const void* x, const void* base, void* new_base, void* packet,
                 int N, int C, int param, int flags, void* workspace, size_t workspace_bytes, void* stream);
int cfx_decompress(cfx_ctx* ctx, int codec, const void* packet, const void* base, void* recon,
                   int N, int C, int param, void* stream);

/* The 2-bit quantise kernel alone, SCALES GIVEN: each item's packet tail already holds tok (N fp16, after the N*C/4 code bytes) and chan
 * (C fp16); codes (+ error-feedback state with CFX_FLAG_UPDATE_CACHE) are written (CFX_FLAG_ELEM_BF16: x, base, new_base bf16).  Replaces the Triton kernel _int2_quant_fastpath
 * (xfuser/compact/fastpath.py:486-580) as the reference launches it behind its eager scale prologue (:614-625) - what a parity test
 * needs to compare codes bit for bit given the reference's own scale vectors. */
int cfx_int2_quantize(cfx_ctx* ctx, int N, int C, int flags, int batch, const cfx_comp_item* items, void* stream);

/* Low-rank residual codecs (compactfusion_amd/csrc/cfx_lowrank.hip).
 *   cfx_lr_compress_batch   replaces subspace_iter (xfuser/compact/compress_lowrank.py:14-61) + the LOW_RANK / LOW_RANK_Q
 *                           encode of slowpath.py:54-75 + the residual / error-feedback flow of main.py:227-233
 *   cfx_lr_decompress_batch replaces slowpath.py:120-131, :151-164 (torch.matmul(u, v), int4 factor dequant) + main.py:376
 * quantized = 0: LOW_RANK   wire [ U (N,r) fp16 | V (r,C) fp16 ]
 * quantized = 1: LOW_RANK_Q wire [ int4(U) (N/2,r) | scale r | min r | int4(V^T) (C/2,r) | scale r | min r ]   (rank % 8 == 0)
 * rank even, <= 32.  init_q[i] -> device C x RP fp32 row-major start matrix, RP = 8/16/32 = rank rounded up, columns >= rank
 * zero; it need not be orthonormal (the iteration only sees its span); its entries enter the first product as fp16 (hi + lo): keep them
 * below 65504 in magnitude (randn is what the reference draws).  Workspace from cfx_lr_workspace_bytes.
 * rank <= 16 on a shard of at most 576 tokens: ONE persistent launch (csrc/cfx_lrslab.hip) whose workgroups wait for each other - taken
 * only where C / 32 workgroups per tensor fit the CUs of `stream` (otherwise a multi-launch chain runs; same results within the codec's
 * tolerance).  It hands its partial sums over through an arena the context owns (allocated on the first call of a stream, zeroed when
 * the shape changes): make one call before capturing the stream into a hipGraph; the launch itself is capturable. */
size_t cfx_lr_packet_bytes(int quantized, int N, int C, int rank);
size_t cfx_lr_workspace_bytes(int quantized, int N, int C, int rank, int batch);
int    cfx_lr_compress_batch(cfx_ctx* ctx, int quantized, int N, int C, int rank, int flags, int batch,
                             const cfx_comp_item* items, const void* const* init_q,
                             void* workspace, size_t workspace_bytes, void* stream);
int    cfx_lr_decompress_batch(cfx_ctx* ctx, int quantized, int N, int C, int rank, int batch,
                               const cfx_decomp_item* items, void* workspace, size_t workspace_bytes, void* stream);

/* 1-bit codec with rank-K scales (COMPACT_COMPRESS_TYPE.BINARY with comp_rank >= 1; deprecated in the reference, main.py:188-189):
 *   cfx_binary_rank_compress_batch   replaces binary_quant_fastpath(rank >= 1) (xfuser/compact/fastpath.py:124-228: subspace_iter(|x - base|)
 *                                    for the scales + the K-loop of _binary_quant_fastpath :88-120) and quantize_1bit(rank >= 1)
 *                                    (compress_quantize.py:37-49)
 *   cfx_binary_rank_decompress_batch replaces binary_dequant_fastpath (fastpath.py:371-438, K-loop :330-360) / dequantize_1bit
 * scale[n, c] = fp16(sum_k fp16(U[n,k] * V[c,k])), out = base + (2 b - 1) * scale.  Wire [ bits N*C/8 | U (N,K) fp16 | V (C,K) fp16 ]
 * (main.py:149-152).  rank 1 .. 32 (the reference's Triton kernels take the powers of two, fastpath.py:91 tl.arange(0, RANK); 32 is the
 * factor chain's limit); init_q[i] as for cfx_lr_compress_batch (device C x {8, 16, 32} fp32 - the rank rounded up -, columns >= rank zero). */
size_t cfx_binary_rank_packet_bytes(int N, int C, int rank);
size_t cfx_binary_rank_workspace_bytes(int N, int C, int rank, int batch);
int    cfx_binary_rank_compress_batch(cfx_ctx* ctx, int N, int C, int rank, int flags, int batch, const cfx_comp_item* items,
                                      const void* const* init_q, void* workspace, size_t workspace_bytes, void* stream);
int    cfx_binary_rank_decompress_batch(cfx_ctx* ctx, int N, int C, int rank, int batch, const cfx_decomp_item* items, void* stream);

/* Native per-launch timing.  When enabled, every `stride`-th launch of a kernel whose id bit is set in kernel_mask
 * is bracketed by hipEvents recorded on the launch stream (up to `capacity` records; capacity 0 disables).  An event
 * pair costs ~2-5 us of stream time, hence the stride.
 * cfx_profile_read synchronises on the recorded events, returns their count and resets the log.
 * Kernel ids: 1 absmean_stats<bits>, 2 absmean_stats, 3 absmean_finalize, 4 binary_dequant, 5 int2_quant,
 * 6 int2_dequant, 7 minmax_stats, 8 minmax_finalize, 9 int8_quant, 10 int8_dequant, 11 int4_quant,
 * 12 int4_dequant, 13 topk_compress, 14 topk_decompress, 15 copy_probe, 16 binary_dequant launched as the
 * sender's error-feedback update, 17-22 low-rank chain (prep, aq, aty, chol, apply, decode), 23 binary_pipe (steady-state
 * fused launch of cfx_plan_run_pipelined), 24 binary_pipe prologue / epilogue / ragged-unit launches, 25 residual2_delta,
 * 26 residual2_update, 27 absmean_compress<bits> (statistics + sign bits + in-launch finalize [+ ride-along reconstruction]),
 * 28 absmean_compress (2-bit statistics + in-launch finalize), 29 minmax_compress (int4 / int8 statistics + in-launch finalize), 30 attn_merge (cfx_attn_merge_ex's and cfx_attn_merge_many's launches too). */
int         cfx_profile_enable(cfx_ctx* ctx, int capacity, unsigned kernel_mask, int stride);
int         cfx_profile_read(cfx_ctx* ctx, int* kernel_ids, float* ms, int cap);
const char* cfx_kernel_name(int kernel_id);

/* Plan: a prebuilt schedule of batch ops (e.g. the 57 layers x {compress, reconstruct} of one denoise step) that is
 * replayed from native code - the MI355X-native replacement for the reference's per-call Python dispatch
 * (xfuser/compact/ring.py:188-206, main.py:169-270).  cfx_plan_add_* copy their arguments and return the op index
 * (>= 0) or an error (< 0); cfx_plan_run launches ops [first_op, first_op + n_ops) on `stream`. */
typedef struct cfx_plan cfx_plan;
cfx_plan* cfx_plan_create(cfx_ctx* ctx);
void      cfx_plan_destroy(cfx_plan* plan);
int       cfx_plan_add_compress(cfx_plan* plan, int codec, int N, int C, int param, int flags, int batch,
                                const cfx_comp_item* items, void* workspace, size_t workspace_bytes);
int       cfx_plan_add_compress_ex(cfx_plan* plan, int codec, int N, int C, int param, int flags, int batch,
                                   const cfx_comp_item* items, int n_ride, const cfx_decomp_item* ride,
                                   void* workspace, size_t workspace_bytes);   /* cfx_compress_batch_ex as a plan op */
int       cfx_plan_add_compress_gated(cfx_plan* plan, int codec, int N, int C, int param, int flags, int batch,
                                      const cfx_comp_item* items, int n_ride, const cfx_decomp_item* ride,
                                      int n_gated, const cfx_decomp_item* gated,
                                      void* workspace, size_t workspace_bytes);   /* cfx_compress_batch_gated as a plan op */
int       cfx_plan_add_decompress(cfx_plan* plan, int codec, int N, int C, int param, int batch,
                                  const cfx_decomp_item* items);
/* cfx_lr_compress_batch / cfx_lr_decompress_batch as plan ops (a LOW_RANK / LOW_RANK_Q layer replayed without per-op marshalling:
 * slowpath.py:54-75, :120-131, :151-164 once per layer of patchpara/fwd.py:108-131).  Pointers (items, init_q, workspace) must stay
 * valid while the plan is replayed. */
int       cfx_plan_add_lr_compress(cfx_plan* plan, int quantized, int N, int C, int rank, int flags, int batch,
                                   const cfx_comp_item* items, const void* const* init_q, void* workspace, size_t workspace_bytes);
int       cfx_plan_add_lr_decompress(cfx_plan* plan, int quantized, int N, int C, int rank, int batch,
                                     const cfx_decomp_item* items, void* workspace, size_t workspace_bytes);
/* Exchange ops.  An all-gather op is ordered after everything the plan enqueued on the main stream before it (the
 * packets are complete); with a side stream (modes 1, 2) a wait op makes the main stream wait for that gather, so
 * "compress(l+1), gather(l+1), wait(l), reconstruct(l)" overlaps the wire with the codec; in mode 0 waits are no-ops. */
typedef struct cfx_comm cfx_comm;
/* where all-gather ops run: 0 = in order on the main stream (default; measured best for layer-sized work, a
 * cross-stream event hop costs ~10 us here), 1 = side stream, 2 = prioritised side stream.  Set before adding ops.
 * cfx_plan_run_pipelined with mode 1 / 2 issues the collectives of unit u on that stream underneath the fused launch that
 * follows finalize(u) (one more unit of look-ahead; no wait ops needed). */
int       cfx_plan_set_exchange_stream(cfx_plan* plan, int mode);
/* Use the caller's stream as this plan's exchange stream (mode 1 semantics; the plan does not own it).  Many plans - one
 * per layer - should share ONE exchange stream: every stream is a hardware queue to the dispatcher. */
int       cfx_plan_use_exchange_stream(cfx_plan* plan, void* stream);
/* layers (1..7, default 7) per unit of cfx_plan_run_pipelined; set before the first replay */
int       cfx_plan_set_pipe_unit_layers(cfx_plan* plan, int layers);
int       cfx_plan_add_all_gather(cfx_plan* plan, cfx_comm* comm, const void* send, void* recv, size_t bytes_per_rank);
int       cfx_plan_add_wait(cfx_plan* plan, int gather_op);
/* Exchange layer: compress ; all-gather ; reconstruct as ONE op - the in-order layer of the gather schedules (reference
 * xfuser/compact/ring.py:188-206 + 265-269, patchpara/fwd.py:108-137: quantise, exchange, dequantise every peer's shard onto its
 * state).  The reconstruction workgroups are launched WITH the compress group on the stream cfx_plan_run is given: they pull their
 * state tiles into registers while the statistics chain and the collective run, and continue when the plan's exchange stream - which
 * waits (a flag kernel) until the launch's packets are complete, issues ncclAllGather(send, recv, bytes_per_rank) and then sets the
 * launch's external gate - says the packets have arrived.  `recon` items read their packets from wherever the collective leaves them
 * (or from this op's own packet operands: with CFX_FLAG_UPDATE_CACHE the rank's own error-feedback update joins them).  comm NULL:
 * nothing moves, the exchange stream runs one relay kernel (wait + set).  Any codec; the one-launch form exists for the 1-bit codec.
 * When the one-launch form is not available (codec or shape
 * without it, a run stream masked below 128 CUs, the legacy NULL stream beside a BLOCKING exchange stream - every CU-masked stream is
 * one -, cfx_hw_queues_ok() == 0, cfx_plan_run_lane) the op runs as compress ; all-gather ; reconstruct in order - same results.  The exchange stream must own a hardware queue (see "Exchange lane" below): the plan creates a
 * CU-masked one unless cfx_plan_use_exchange_stream supplied it (one stream should serve all plans).  A gate that never opens times
 * out like any flag wait (CFX_ERR_GATE at the next call).
 * With more than one rank the collective is a KERNEL that has to be placed while the reconstruction workgroups hold their CUs: the
 * one-launch form is then taken only if that group leaves 32 workgroup slots of the run stream's CUs free (room for RCCL's workgroups:
 * 256 threads x ~280 VGPRs on gfx950), otherwise the op runs in order.  Returns the op index. */
int       cfx_plan_add_exchange_layer(cfx_plan* plan, int codec, int N, int C, int param, int flags, int batch,
                                      const cfx_comp_item* items, int n_recon, const cfx_decomp_item* recon,
                                      cfx_comm* comm, const void* send, void* recv, size_t bytes_per_rank,
                                      void* workspace, size_t workspace_bytes);
/* The exchange layer WITHOUT a collective, for the GPUs of one node: every rank's packets stay where the compress launch wrote them - in
 * a buffer from cfx_ipc_alloc that the peers have opened with cfx_ipc_open - and a peer's reconstruction workgroups read them from
 * there over xGMI (`recon` items point into the opened mappings).  What is exchanged is one 4-byte word per rank and layer, and the exchange
 * runs INSIDE the launch: workgroup 0, once its own tile is done, waits until the launch's packets are complete, advances *own_flag by one
 * (the op's execution count 1, 2, ... - taken from the word itself on the device, so a rebuilt plan keeps counting where the words stand;
 * every rank executes the same ops equally often), waits until every peer_flags[i] has reached that count and opens the launch's gate.  ONE
 * launch per layer on ONE stream: no exchange stream, no collective kernel that has to find CUs beside the waiting workgroups, no
 * hardware-queue requirement, any run stream (the legacy NULL stream included).  own_flag and the peers' flags live in cfx_ipc_alloc memory
 * (zero-initialised), one word per op and plan; a rank may rewrite a layer's packets only after its peers have moved past that layer: a plan
 * has at least two such ops per replay, or the caller double-buffers packets and flag words by execution parity (compact/xlayer.py).
 * Replaces the all-gather of ring.py:188-206 / patchpara/fwd.py:108-109 on a single node.  1-bit, 2-bit, int4, int8 (the min/max and 2-bit
 * codecs where all their statistics workgroups are co-resident); otherwise - shape / stream without the one-launch form - compress ; a
 * one-wave kernel that publishes and waits ; reconstruct in stream order: same results.  Time-outs as for cfx_plan_add_exchange_layer. */
#define CFX_P2P_MAX_PEERS 15
int       cfx_plan_add_exchange_layer_p2p(cfx_plan* plan, int codec, int N, int C, int param, int flags, int batch,
                                          const cfx_comp_item* items, int n_recon, const cfx_decomp_item* recon,
                                          void* own_flag, int n_peers, const void* const* peer_flags,
                                          void* workspace, size_t workspace_bytes);
/* The publish-and-wait step of the p2p exchange as an op of its own, for chains that keep separate launches (compress ; p2p_sync ;
 * reconstruct peer 1 ; reconstruct peer 2 ; ... - the lane plan of compact_fwd): runs in stream order where the op range runs; what
 * the ops before it wrote is complete when *own_flag is published, the ops behind it start after every peer has published.  Flags
 * as in cfx_plan_add_exchange_layer_p2p (one word per op and plan, cfx_ipc_alloc memory, execution count as the epoch). */
int       cfx_plan_add_p2p_sync(cfx_plan* plan, void* own_flag, int n_peers, const void* const* peer_flags);
/* Device memory shared between the processes of a node (hipIpcGetMemHandle / hipIpcOpenMemHandle; on hosts with dmabuf IPC only the
 * processes need HSA_ENABLE_IPC_MODE_LEGACY=0).  cfx_ipc_alloc: zeroed device memory + its 64-byte handle (send it to the peers by any
 * means); cfx_ipc_open: map a peer's allocation; close / free when done.
 * The memory is UNCACHED device memory (hipExtMallocWithFlags(hipDeviceMallocUncached); fine-grained, then ordinary memory as fall-backs,
 * cfx_ipc_memory_kind says which): peers poll words in it and read packets from it while the producing kernel is still running, and the
 * same addresses are rewritten every step - ordinary device memory is only promised coherent across devices at kernel boundaries. */
int       cfx_ipc_alloc(cfx_ctx* ctx, size_t bytes, void** ptr, void* handle64);
int       cfx_ipc_memory_kind(cfx_ctx* ctx);   /* what the last cfx_ipc_alloc of the context returned: 2 uncached, 1 fine-grained, 0 ordinary */
int       cfx_set_ipc_memory_kind(cfx_ctx* ctx, int kind);   /* what cfx_ipc_alloc asks for first (default 2; measurements: 1, 0) */
int       cfx_ipc_open(cfx_ctx* ctx, const void* handle64, void** ptr);
int       cfx_ipc_close(cfx_ctx* ctx, void* ptr);
int       cfx_ipc_free(cfx_ctx* ctx, void* ptr);
/* One hop of the ring relay (reference xfuser/compact/ring.py:193-195,265-269: RingComm.send_recv / commit / wait): send
 * `bytes` to rank+1 and receive `bytes` from rank-1 as one grouped ncclSend + ncclRecv, on the exchange stream like an
 * all-gather op (cfx_plan_add_wait applies).  W-1 hops relay every rank's packet around the ring. */
int       cfx_plan_add_ring_hop(cfx_plan* plan, cfx_comm* comm, const void* send, void* recv, size_t bytes);
/* Re-point the activation of item `item` of compress op `op` (the K / V tensor a layer hands over changes from call to
 * call; state, packet and workspace operands are bound once). */
int       cfx_plan_set_input(cfx_plan* plan, int op, int item, const void* x);
int       cfx_plan_size(const cfx_plan* plan);
int       cfx_plan_copy_op(cfx_plan* dst, const cfx_plan* src, int op);   /* append a copy of a (de)compress op of `src` */
int       cfx_plan_run(cfx_plan* plan, int first_op, int n_ops, void* stream);
/* cfx_plan_run after re-pointing the n_xs activations of the first compress op of the range (cfx_plan_set_input + run in
 * one host call: what a layer's K,V hand-over costs). */
int       cfx_plan_run_x(cfx_plan* plan, int first_op, int n_ops, const void* const* xs, int n_xs, void* stream);
/* Exchange lane: the layer's chain (compress, collective, per-peer reconstruction) on its own - normally CU-masked - stream, ordered
 * with the compute stream ONLY through flag words in device memory (no events: a cross-stream event hop costs ~14 us of idle queue
 * time on MI355X / ROCm 7.2, a flag written by one stream's kernel and polled by the other's ~1.7 us; tools/lane_probe.hip).
 * Replaces the reference's fork / join of the K,V exchange around the local attention block (xfuser/compact/ring.py:191-269:
 * RingComm.send_recv + commit before the block, wait after it, decompress on the compute stream).
 *   cfx_plan_flags(plan, n)       allocates the plan's n flag words (64 bytes apart, zeroed; once per plan) and returns the device
 *                                 address of flag 0, or NULL.  Flags hold monotonic EPOCHS: one per cfx_plan_run_lane call.
 *   cfx_plan_add_flag_wait / _set plan ops: wait until flag i has reached the current epoch / set flag i to it.  A set op makes
 *                                 everything the ops before it wrote visible to whoever waits (kernel boundary in an in-order stream).
 *   cfx_plan_run_lane             advances the epoch, launches "set flag `ready_flag`" on `compute_stream` (behind the kernels that
 *                                 produce the activations xs, see cfx_plan_run_x) and replays the op range on the plan's exchange
 *                                 stream (cfx_plan_use_exchange_stream); the range normally starts with a wait op on `ready_flag`.
 *                                 *epoch_out receives the epoch the range's set ops will publish.  One host call per layer.
 *   cfx_attn_merge_wait           cfx_attn_merge whose launch also waits (one lane, after its merge work) until *wait_flag has
 *                                 reached wait_value: the attention block that follows it in the compute stream then finds the
 *                                 peer's reconstructed K,V complete.  wait_flag NULL = cfx_attn_merge.
 *   cfx_flag_set / cfx_flag_wait  the same two tiny kernels for callers that order other work (flag = any 4-byte-aligned device word).
 * A wait gives up after the context's gate timeout (default 5 s, cfx_set_gate_timeout_ms) and counts the failure in a pinned host
 * word: the next plan / compress / merge call on the context returns CFX_ERR_GATE, cfx_gate_errors reads and clears the count
 * without synchronising the device.
 * The two streams a flag orders must NOT share a hardware queue (the polling kernel would block the kernel it waits for until the
 * timeout): HIP multiplexes ordinary streams over a small pool of queues, a CU-masked stream owns its queue - create at least the
 * exchange stream with cfx_stream_create_masked (a full mask, first_cu = 0, n_cus = all, is fine).
 *   cfx_stream_create_masked      a stream restricted to CU-mask bits [first_cu, first_cu + n_cus) (hipExtStreamCreateWithCUMask; on
 *                                 MI355X bit i = CU i/8 of XCD i%8, so a contiguous range is the same share of every XCD).  The lane
 *                                 uses two with DISJOINT ranges - e.g. 32 CUs for the exchange, 224 for the compute stream the
 *                                 attention kernels run on - so that neither slows the other's workgroups (tools/sdpa_mask_probe.py:
 *                                 SDPA 37 us alone, 38 us beside a saturating copy on the other 32 CUs, 93 us when it shares them). */
void*     cfx_plan_flags(cfx_plan* plan, int n);
int       cfx_plan_add_flag_wait(cfx_plan* plan, int flag);
int       cfx_plan_add_flag_set(cfx_plan* plan, int flag);
int       cfx_plan_set_pre_flag(cfx_plan* plan, int op, int flag);   /* reconstruction op `op` sets `flag` as the first thing its launch
                                                                       * does (= after the op in front of it, without a launch of its own) */
unsigned  cfx_plan_epoch(const cfx_plan* plan);
int       cfx_plan_run_lane(cfx_plan* plan, int first_op, int n_ops, const void* const* xs, int n_xs, int ready_flag,
                            void* compute_stream, unsigned* epoch_out);
/* cfx_plan_run_lane's first half on its own: advance the epoch and launch "set flag `ready_flag`" on `compute_stream`.  A later
 * cfx_plan_run_lane with compute_stream = NULL then only replays the op range (same epoch): the caller enqueues the local attention
 * block in between, so the chain's host issue overlaps GPU work. */
int       cfx_plan_lane_begin(cfx_plan* plan, int ready_flag, void* compute_stream, unsigned* epoch_out);
int       cfx_flag_set(cfx_ctx* ctx, void* flag, unsigned value, void* stream);
int       cfx_flag_wait(cfx_ctx* ctx, const void* flag, unsigned value, void* stream);
int       cfx_stream_create_masked(cfx_ctx* ctx, int first_cu, int n_cus, void** stream);
int       cfx_stream_destroy(cfx_ctx* ctx, void* stream);
int       cfx_set_gate_timeout_ms(cfx_ctx* ctx, int ms);
/* Software-pipelined replay (replaces the reference's strictly sequential quantise -> cat -> send -> dequantise per layer,
 * xfuser/compact/ring.py:188-260 with fastpath.py:124-228, 371-438).  If ops [first_op, first_op + n_ops) are a sequence of "groups"
 *     k x compress (BINARY, flags without UPDATE_CACHE)   { all-gather }*   k x decompress (BINARY)      of one shape,
 * (k >= 1 layers whose packets travel in one collective) consecutive groups are merged into units of up to 7 layers
 * (cfx_plan_set_pipe_unit_layers; at most 112 reconstruction and 16 compress items per unit) and replayed on `stream` as
 *     { all-gathers of unit t-2 } ; [dequant(unit t-2) | finalize(unit t-1) | stats(unit t)]          t = 0, 1, ...
 * with every bracket ONE fused launch, so the small statistics kernels of later layers run underneath the
 * reconstruction of earlier ones.  Results are bit-identical to cfx_plan_run; packet / state buffers must be distinct
 * per layer within the call; the statistics workspaces are plan-owned (the ops' own are not used).  Any other op
 * sequence is replayed by cfx_plan_run. */
int       cfx_plan_run_pipelined(cfx_plan* plan, int first_op, int n_ops, void* stream);
/* Call once after the last cfx_plan_add_*: recognises the unit schedule of the whole plan for cfx_plan_run_pipelined and
 * makes every allocation a replay needs (statistics workspaces, the context's ticket blocks), so that cfx_plan_run /
 * cfx_plan_run_pipelined do no host allocation, environment lookup or device allocation per step (optional: the first
 * replay of a range does the same work otherwise). */
int       cfx_plan_finalize(cfx_plan* plan);

/* Process-global state, the only one besides cfx_ctx: the table of RCCL entry points filled by cfx_rccl_load (RCCL is a
 * process-wide library; loading it twice would give two collective runtimes).  Communicators themselves are per cfx_comm.
 * cfx_comm_create leaves the caller's current device unchanged.
 * RCCL communicator owned by the library (replaces yunchang's RingComm + torch.distributed P2P of the reference,
 * xfuser/compact/ring.py:172,193-195,265-267).  RCCL is loaded at run time (cfx_rccl_load: pass the path of the
 * librccl the process already uses, or NULL to search); rank 0 makes the 128-byte unique id (cfx_comm_unique_id),
 * the host shares it by any means, every rank calls cfx_comm_create (collective). */
int       cfx_rccl_load(const char* path);   /* a different explicit path replaces the table for communicators created afterwards */
int       cfx_comm_unique_id(cfx_ctx* ctx, void* out128);
cfx_comm* cfx_comm_create(cfx_ctx* ctx, const void* id128, int nranks, int rank);
void      cfx_comm_destroy(cfx_comm* comm);
int       cfx_comm_all_gather(cfx_comm* comm, const void* send, void* recv, size_t bytes_per_rank, void* stream);
int       cfx_comm_ring_hop(cfx_comm* comm, const void* send, void* recv, size_t bytes, void* stream);

/* Second-order residual (CompactConfig(residual=2), xfuser/compact/main.py:244-266 compress, :378-384 decompress): the
 * predictor arithmetic around any codec, n fp16 elements (multiple of 8), one fp16 rounding per reference operation.
 *   cfx_residual2_delta :  dd = (x - base) - delta_base                        -> compress dd with base = NULL
 *   cfx_residual2_update:  new_base = (base + delta_base) + recv ; new_delta_base = fp16(fp32(fp16(delta_base + recv)) * decay)
 * (recv = decode(packet) with base = NULL; decay = CompactConfig.delta_decay_factor, main.py:272-273).  new_base may alias
 * base and new_delta_base may alias delta_base. */
int cfx_residual2_delta(cfx_ctx* ctx, const void* x, const void* base, const void* delta_base, void* dd, size_t n, void* stream);
int cfx_residual2_update(cfx_ctx* ctx, const void* base, const void* delta_base, const void* recv, void* new_base,
                         void* new_delta_base, float decay, size_t n, void* stream);

/* The second-order predictor INSIDE the 1-bit and 2-bit codec launches ("Second-order residual" above): second[i] belongs to items[i].
 * cfx_compress_batch_res2 = cfx_compress_batch with the codec seeing (x - base) - delta_base and, with CFX_FLAG_UPDATE_CACHE, both states
 * updated from the call's own packet; cfx_decompress_batch_res2 = cfx_decompress_batch writing recon = (base + delta_base) + recv and,
 * where new_delta_base is given, the decayed second-order state.  Checks in the order of the first-order calls (null ctx / items /
 * second, batch, codec / shape, per item: null, alignment; workspace), the second-order refusals (CFX_FLAG_NO_EF, CFX_ELEM_BF16,
 * codec ids 3 - 5: CFX_ERR_CODEC) with the codec check.  Capturable as the ungated first-order calls are. */
typedef struct cfx_second_item {
    const void* delta_base;     /* (N,C) fp16, 16-byte aligned: required */
    void*       new_delta_base; /* (N,C) fp16, 16-byte aligned; may alias delta_base; NULL (reconstruction items): not written */
} cfx_second_item;
int cfx_compress_batch_res2(cfx_ctx* ctx, int codec, int N, int C, int param, int flags, int batch, const cfx_comp_item* items,
                            const cfx_second_item* second, float decay, void* workspace, size_t workspace_bytes, void* stream);
int cfx_decompress_batch_res2(cfx_ctx* ctx, int codec, int N, int C, int param, int batch, const cfx_decomp_item* items,
                              const cfx_second_item* second, float decay, void* stream);
/* Attach second-order states to plan op `op`, built by cfx_plan_add_compress, cfx_plan_add_decompress, cfx_plan_add_exchange_layer or
 * cfx_plan_add_exchange_layer_p2p (1-bit / 2-bit, fp16, no CFX_FLAG_NO_EF, no ride-along or gated items: CFX_ERR_CODEC otherwise),
 * before cfx_plan_finalize.  comp_second[n_comp] belong to the op's compress items (n_comp = its batch; 0 for a reconstruction op),
 * rec_second[n_rec] to its reconstruction items (the op's batch for a reconstruction op, n_recon for an exchange layer, 0 for a compress
 * op); any other count, an op index out of range or another kind of op is CFX_ERR_BATCH.  The op then runs the second-order launches;
 * an exchange layer with states attached never takes a one-launch layer form: compress ; exchange ; reconstruct in stream order (the
 * peer-to-peer word exchange as a one-wave kernel), same results.  cfx_plan_copy_op copies the states with the op, cfx_plan_set_input
 * and cfx_plan_run_x re-point its activations as before. */
int cfx_plan_set_second_order(cfx_plan* plan, int op, int n_comp, const cfx_second_item* comp_second, int n_rec,
                              const cfx_second_item* rec_second, float decay);

/* Ring-attention block merge - the consumer side of the exchange (reference xfuser/compact/ring.py:263 calls
 * yunchang.ring.utils.update_out_and_lse, un-vendored; published formula):
 *   out <- out - sigmoid(lse_b - lse) * (out - out_b) ;  lse <- lse - logsigmoid(lse - lse_b)         (fp32)
 * out fp32 [B][S][H][D], lse fp32 [B][S][H]; block_out fp16 [B][H][S][D] (block_out_bshd = 0) or [B][S][H][D] (= 1), block_lse fp32 [B][H][S]
 * (the fused SDPA kernel's own output layouts).  first != 0 initialises out / lse from the block.  D % 8 == 0.  One launch per block instead of ~10
 * eager elementwise kernels. */
int cfx_attn_merge(cfx_ctx* ctx, void* out, void* lse, const void* block_out, const void* block_lse, int B, int S, int H, int D,
                   int block_out_bshd, int first, void* stream);
int cfx_attn_merge_wait(cfx_ctx* ctx, void* out, void* lse, const void* block_out, const void* block_lse, int B, int S, int H, int D,
                        int block_out_bshd, int first, const void* wait_flag, unsigned wait_value, void* stream);
/* The same merge for fp16 OR bf16 blocks, with the layer's final cast in the launch.  `flags`: CFX_MERGE_BSHD (block_out is
 * [B][S][H][D]; otherwise [B][H][S][D]), CFX_MERGE_FIRST (initialise from the block), CFX_ELEM_BF16 (block_out - and final_out - are
 * bf16: widened to fp32 exactly, the arithmetic is the same fp32 arithmetic); any other bit is CFX_ERR_CODEC.  wait_flag / wait_value
 * as in cfx_attn_merge_wait.
 *   final_out == NULL   out / lse are updated exactly as cfx_attn_merge_wait updates them.
 *   final_out != NULL   the layer's LAST block: the merged result - the very fp32 values the other form would have stored in `out` -
 *                       is rounded to the element type (nearest even) and written to final_out, a contiguous [B][S][H][D] 16-bit
 *                       tensor; lse is updated as usual, `out` is only read.  With CFX_MERGE_FIRST (a single block) final_out takes
 *                       the block's own bits, lse the block's, and `out` is not touched: it may then be NULL.
 * Checks, in this order: a NULL pointer CFX_ERR_NULL, an unknown flag bit CFX_ERR_CODEC, the shape (D % 8 == 0, D <= 512)
 * CFX_ERR_SHAPE, 16-byte alignment of out, block_out and final_out CFX_ERR_ALIGN, a pending gate error CFX_ERR_GATE.  Finite inputs. */
#define CFX_MERGE_BSHD 1
#define CFX_MERGE_FIRST 2
int cfx_attn_merge_ex(cfx_ctx* ctx, void* out, void* lse, const void* block_out, const void* block_lse, int B, int S, int H, int D,
                      int flags, const void* wait_flag, unsigned wait_value, void* final_out, void* stream);

/* ALL of a layer's blocks merged in ONE launch: the softmax-weighted combination of n blocks (1 <= n <= CFX_MERGE_MAX_BLOCKS) formed
 * directly, not as a chain of cfx_attn_merge_ex calls - every block's output is read once, the result written once.
 *   block_outs[i]   fp16 (bf16 with CFX_ELEM_BF16) [B][H][S][D], or [B][S][H][D] with CFX_MERGE_BSHD (all blocks alike), 16-byte aligned
 *   block_lses[i]   fp32 [B][H][S]
 *   out             with CFX_MERGE_OUT_F32: fp32 [B][S][H][D] - what the chain leaves in its accumulator; without: the same fp32 value
 *                   rounded to the element type (nearest even) into a contiguous 16-bit [B][S][H][D] tensor, the layer's result
 *   lse             fp32 [B][S][H]
 * The two tables are HOST arrays of n device pointers, copied into the launch's arguments: nothing is allocated or written on the
 * device besides out / lse, and the launch can be captured into a hipGraph (the graph holds the pointers).  out / lse alias no input.
 * Arithmetic, per row (b, s, h), in fp32, every operation rounded once, none contracted:
 *   m     = max_i lse_i
 *   x_i   = lse_i - m                       one subtraction (0 for the maximum)
 *   e_i   = exp(x_i)                        the fast exponential (2^(fp32(log2 e) x_i), rounded product); exactly 1 for the maximum
 *   Z     = ((e_0 + e_1) + e_2) + ...       n - 1 additions in index order
 *   a_d   = ((e_0 o_0d + e_1 o_1d) + ...)   each product rounded, n - 1 additions in index order
 *   out_d = a_d / Z                         one correctly rounded DIVISION (not a reciprocal and a product)
 *   lse   = m + logf(Z)                     one logarithm, one addition
 * n = 1 returns the block's own values and lse exactly (e = 1, Z = 1, logf(1) = 0).  Finite inputs.
 * `flags`: CFX_MERGE_BSHD, CFX_ELEM_BF16, CFX_MERGE_OUT_F32; CFX_MERGE_FIRST is not accepted here.  Checks, in this order: a NULL pointer -
 * entries of the two tables included - CFX_ERR_NULL, an unknown flag bit CFX_ERR_CODEC, n outside 1 .. 16 or the shape (D % 8 == 0,
 * D <= 512) CFX_ERR_SHAPE, 16-byte alignment of out and of every block_outs[i] CFX_ERR_ALIGN, a pending gate error CFX_ERR_GATE.  The
 * launch reports as kernel id 30 (attn_merge) in cfx_profile_read: ONE record where the chain leaves n. */
#define CFX_MERGE_MAX_BLOCKS 16
#define CFX_MERGE_OUT_F32 4
int cfx_attn_merge_many(cfx_ctx* ctx, int n, const void* const* block_outs, const void* const* block_lses,
                        int B, int S, int H, int D, int flags, void* out, void* lse, void* stream);

/* Native ring-attention forward: the attention of a rank's queries over ALL of a layer's K,V blocks in ONE launch - non-causal, no
 * dropout -, the blocks read where they lie through two pointer tables: no concatenation, no per-block out / lse, no merge.
 *   q               fp16 (bf16 with CFX_ELEM_BF16: every tensor alike) [B][Sq][H][D] contiguous, 16-byte aligned; D = 64 or 128
 *   ks[i], vs[i]    i < n, 1 <= n <= CFX_ATTN_MAX_BLOCKS: [B][Sk][H][D] contiguous, 16-byte aligned, ONE Sk for all blocks - the
 *                   arena's (N, C) state layout with C = H D.  The keys of the blocks count as one sequence, in table order
 *   out             [B][Sq][H][D] in the element type;  lse  fp32 [B][Sq][H] (natural logarithm), both 16-byte aligned
 * The two tables are HOST arrays of n device pointers, copied into the launch's arguments: nothing is allocated or written on the device
 * besides out / lse, and the launch can be captured into a hipGraph (the graph holds the pointers).  out / lse alias no input.  The
 * launch waits for nothing: every block must be complete in stream order (cfx_flag_wait in front of it where a lane produces them).
 * Sq and Sk are arbitrary positive numbers.  A workgroup owns 128 consecutive query rows of one (b, h) - a wave 32 - and walks the
 * blocks in table order in tiles of 64 keys with one running (m, l, O) per row; keys past a block's end are masked.
 * Arithmetic, per query row, every fp32 operation rounded once, none contracted; j runs over a tile's keys:
 *   a_j   = sum_d q_d k_jd                  fp32 accumulation of the EXACT 16-bit products (v_mfma_f32_32x32x16), hardware order
 *   t_j   = a_j * softmax_scale             one fp32 product; a masked key: t_j = -inf
 *   m'    = max(m, max_j t_j)               updated at EVERY tile (no deferred maximum); m = -inf before the first tile
 *   f     = exp(m - m')                     the fast exponential, 2^(fp32(log2 e) x) with the product rounded: 0 at the first tile, exactly
 *                                           1 when the maximum stands
 *   p_j   = exp(t_j - m')                   one subtraction, the same exponential; exactly 1 for the maximum, 0 for a masked key
 *   l     = l * f + sum_j p_j               from the UNROUNDED p_j, fp32 additions: a lane adds its 32 keys of the tile in register order
 *                                           (two lanes share a row and are added once, at the end)
 *   O_d   = O_d * f + sum_j P_j v_jd        O_d * f one rounding per tile (skipped where f = 1 for a whole wave: the same value);
 *                                           P_j = p_j rounded to the element type (nearest even), the products exact, the fp32
 *                                           accumulation in hardware order
 *   out_d = O_d / l                         ONE correctly rounded division, then one rounding to the element type (nearest even)
 *   lse   = m + logf(l)
 * n = 1, Sk = 1: p = 1, l = 1 - out is v's own bits, lse = a * softmax_scale.  Finite inputs.  Query rows past Sq are computed on zero
 * queries and never stored.
 * `flags`: CFX_ELEM_BF16 only.  Checks, in this order: a NULL pointer - entries of the two tables included - CFX_ERR_NULL; an unknown
 * flag bit CFX_ERR_CODEC; n outside 1 .. 16, a non-positive size, D other than 64 or 128, more workgroups than a launch takes, a scale
 * that is not finite and positive CFX_ERR_SHAPE; q, out, lse or a block not 16-byte aligned CFX_ERR_ALIGN; a pending gate error
 * CFX_ERR_GATE.  Each returns before anything is launched.
 * The 32-bit kernel-id mask of cfx_profile_enable is full: the launch carries NO kernel id and is not recorded there.  The context
 * counts the launches it enqueued instead; cfx_attn_fwd_launches reads the count (a captured launch counts once, its replays not). */
#define CFX_ATTN_MAX_BLOCKS 16
int cfx_attn_fwd_blocks(cfx_ctx* ctx, int n, const void* q, const void* const* ks, const void* const* vs, int B, int Sq, int Sk, int H, int D,
                        float softmax_scale, unsigned flags, void* out, void* lse, void* stream);
/* cfx_attn_fwd_blocks for K,V blocks of UNEQUAL length: block i is [B][sks[i]][H][D] contiguous (its batch stride is its own), sks a HOST
 * array of n key counts copied, like the two pointer tables, into the launch's arguments; every other argument is cfx_attn_fwd_blocks's.
 * What it is for: a layer's joint (text) keys beside its image shards, and queries [text ; image shard] with Sq != sks[i].
 * The keys of the blocks count as one sequence in table order and the arithmetic is the contract above, rounding by rounding.  Tiles are
 * 64 keys and never straddle a block: block i has ceil(sks[i] / 64) of them, the launch walks T = sum_i ceil(sks[i] / 64); keys past a
 * block's OWN end are staged as zeros and scored -inf.  With equal lengths the result is cfx_attn_fwd_blocks's bit for bit; blocks whose
 * lengths are multiples of 64 give the bits of ONE block that holds their keys in order (the same tile sequence).
 * Nothing is allocated or written on the device besides out / lse; the launch is capturable and waits for nothing.
 * `flags`: CFX_ELEM_BF16 only.  Checks, in this order: a NULL pointer - sks and entries of the two tables included - CFX_ERR_NULL; an
 * unknown flag bit CFX_ERR_CODEC; n outside 1 .. 16, a non-positive B / Sq / H or sks[i], D other than 64 or 128, more workgroups than a
 * launch takes, a scale that is not finite and positive CFX_ERR_SHAPE; q, out, lse or a block not 16-byte aligned CFX_ERR_ALIGN; a
 * pending gate error CFX_ERR_GATE.  Each returns before anything is launched.  The launch carries no kernel id: it counts in
 * cfx_attn_fwd_launches, and cfx_set_attn_qtile sets its query tile too. */
int cfx_attn_fwd_blocks_var(cfx_ctx* ctx, int n, const void* q, const void* const* ks, const void* const* vs, const int* sks,
                            int B, int Sq, int H, int D, float softmax_scale, unsigned flags, void* out, void* lse, void* stream);
/* cfx_attn_fwd_blocks_var for the head dims BETWEEN 64 and 128: D = 72, 80, 88, 96, 104, 112 or 120 (PixArt / Latte run heads of 72,
 * HunyuanDiT of 88).  Every argument and every layout is cfx_attn_fwd_blocks_var's - rows of D elements, no padding: a row is D / 8
 * 16-byte chunks -; a caller with blocks of one length passes sks[i] = Sk.  The arithmetic is the contract above, rounding by rounding,
 * with d running over the TRUE D: the launch takes ceil(D / 16) MFMA k-steps to the scores and ceil(D / 32) accumulator blocks to O, and
 * every operand past column D is an exact zero that is never loaded - a zero product adds nothing to an fp32 sum and rounds nothing.  So
 * out and lse are, bit for bit, out[..., :D] and lse of cfx_attn_fwd_blocks_var on q and the blocks zero-padded to D = 128 with the same
 * softmax_scale.  Nothing within or past a row is read beyond its D elements.  Tiles, masking, the walk's order: cfx_attn_fwd_blocks_var's.
 * Nothing is allocated or written on the device besides out / lse; the launch is capturable and waits for nothing.
 * `flags`: CFX_ELEM_BF16 only.  Checks, in cfx_attn_fwd_blocks_var's order: a NULL pointer - sks and entries of the two tables included -
 * CFX_ERR_NULL; an unknown flag bit CFX_ERR_CODEC; n outside 1 .. 16, a non-positive B / Sq / H or sks[i], D other than the seven above
 * (64 and 128 included: they are cfx_attn_fwd_blocks_var's), more workgroups than a launch takes, a scale that is not finite and
 * positive CFX_ERR_SHAPE; q, out, lse or a block not 16-byte aligned CFX_ERR_ALIGN; a pending gate error CFX_ERR_GATE.  Each returns
 * before anything is launched.  The launch carries no kernel id: it counts in cfx_attn_fwd_launches, and cfx_set_attn_qtile sets its
 * query tile too (the same bits whatever the tile). */
int cfx_attn_fwd_blocks_hd(cfx_ctx* ctx, int n, const void* q, const void* const* ks, const void* const* vs, const int* sks,
                           int B, int Sq, int H, int D, float softmax_scale, unsigned flags, void* out, void* lse, void* stream);
int cfx_attn_fwd_launches(cfx_ctx* ctx, unsigned long long* n);
/* Query rows a workgroup of cfx_attn_fwd_blocks owns: 64, 128 or 256 (2, 4 or 8 waves), 0 = the library's choice (128: measured best on
 * the FLUX shard).  The result is the same function of the inputs whatever the tile; anything else is CFX_ERR_SHAPE.  For
 * measurement (tools/attn_rows.py). */
int cfx_set_attn_qtile(cfx_ctx* ctx, int rows);

/* Bandwidth probe: dst[i] = src[i] over `bytes` (multiple of 16) - the achievable-HBM reference
 * against which bench.py reports roofline fractions. */
int cfx_copy_probe(cfx_ctx* ctx, void* dst, const void* src, size_t bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CFX_H */
