"""Lane-level simulation of wgrad_kernel's index map (csrc/wgrad.hip) on the CPU: the [token][feature] LDS image with its padded row pitch, the
addresses each lane hands to ds_read_b64_tr_b16 (within a 16-lane group, lane 4 q + p supplies row q, columns 4 p ... 4 p + 3 of a 4 x 16 block and lane i
receives column i, row q in element q), the A / B operand maps and the accumulator map of v_mfma_f32_32x32x16, the slab split and the bounds of the
epilogue — restated here from the kernel, with the exact-integer operands of tests/test_gpu_wgrad.py.  It pins the DESIGN of the map (A and B agree on
the token permutation, nothing outside the operands is read as data, every output element is written once per slab); the GPU test pins the kernel."""
import numpy as np
import pytest


def sim(m, n, k, BK, S):
    BN, KT = 128, 64
    PA, PB = BN*2+64, BK*2+64
    dy = ((3*np.arange(m)[:,None] + 5*np.arange(n)[None,:]) % 7 - 3).astype(np.int64)
    x = ((np.arange(m)[:,None] + 2*np.arange(k)[None,:]) % 5 - 2).astype(np.int64)
    slab_rows = (-(-(-(-m//S))//KT))*KT
    out = np.zeros((n,k), np.int64)
    nt, kt = -(-n//BN), -(-k//BK)
    for slab in range(S):
      for tn in range(nt):
        for tk in range(kt):
          n0,k0 = tn*BN, tk*BK
          rb, re = slab*slab_rows, min(m, slab*slab_rows+slab_rows)
          acc = np.zeros((4,2,BK//64,64,16), np.int64)   # wave,i,j,lane,reg
          for row in range(rb, re, KT):
            sa = np.full(KT*PA//2, 999999, np.int64); sb = np.full(KT*PB//2, 999999, np.int64)  # in 16-bit elements
            for W,s,P,src,c0,cols in ((BN,sa,PA,dy,n0,n),(BK,sb,PB,x,k0,k)):
              CH=W//8
              for c in range(KT*CH):
                r = row + c//CH; col = c0 + (c%CH)*8
                v = src[r, col:col+8] if (r<re and col<cols) else np.zeros(8,np.int64)
                off = ((c//CH)*P + (c%CH)*16)//2
                s[off:off+8] = v
            def tr(s, byteaddr):  # byteaddr[64] -> result [64][4]
              res = np.zeros((64,4), np.int64)
              for g in range(4):
                for i in range(16):
                  for q in range(4):
                    a = byteaddr[16*g + 4*q + i//4] // 2   # lane 4q+p supplies row q cols 4p..4p+3; lane i gets col i -> p=i//4, elem i%4
                    res[16*g+i, q] = s[a + i%4]
              return res
            lane = np.arange(64); g = lane>>4; q=(lane&15)>>2; pp=lane&3
            tr_row = 8*(g>>1)+q; tr_col = 16*(g&1)+4*pp
            for wave in range(4):
              wn, wk = wave>>1, wave&1
              a_rd = tr_row*PA + (wn*64+tr_col)*2
              b_rd = tr_row*PB + (wk*(BK//2)+tr_col)*2
              for s_ in range(4):
                fa = [np.concatenate([tr(sa, a_rd+(16*s_)*PA+i*64), tr(sa, a_rd+(16*s_+4)*PA+i*64)],1) for i in range(2)]
                fb = [np.concatenate([tr(sb, b_rd+(16*s_)*PB+j*64), tr(sb, b_rd+(16*s_+4)*PB+j*64)],1) for j in range(BK//64)]
                for i in range(2):
                  for j in range(BK//64):
                    # A[row r][k=8h+jj] in lane (r,h) elem jj ; B[k][col r]
                    A = np.zeros((32,16),np.int64); B = np.zeros((16,32),np.int64)
                    for l in range(64):
                      r_,h=l&31,l>>5
                      A[r_,8*h:8*h+8]=fa[i][l]; B[8*h:8*h+8,r_]=fb[j][l]
                    D = A@B
                    for l in range(64):
                      for reg in range(16):
                        acc[wave,i,j,l,reg] += D[(reg&3)+8*(reg>>2)+4*(l>>5), l&31]
          for wave in range(4):
            wn,wk=wave>>1,wave&1
            for i in range(2):
              for j in range(BK//64):
                for l in range(64):
                  col = k0+wk*(BK//2)+j*32+(l&31)
                  for reg in range(16):
                    nrow = n0+wn*64+i*32+(reg&3)+8*(reg>>2)+4*(l>>5)
                    if nrow<n and col<k: out[nrow,col]+=acc[wave,i,j,l,reg]
    return np.array_equal(out, dy.T@x)


@pytest.mark.parametrize("slabs", [1, 2])
@pytest.mark.parametrize("m,n,k", [(16, 32, 32), (64, 72, 40), (200, 136, 264)])
def test_wgrad_index_map_reproduces_the_integer_product(m, n, k, slabs):
    assert sim(m, n, k, 64 if k <= 64 else 128, slabs)
