#!/usr/bin/env python3
"""The s_waitcnt vmcnt(..) picture of the pipelined row-type product's chunk loop (spmv_dict2_kernel, UNI instantiations),
read from gfx950 assembly:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S saddle_point_petsc_amd/csrc/spk_k_dict.hip -o new.s
    python tools/product_waits.py old.s new.s          (old.s: the same command on the commit to compare with)

Per kernel: the waits at the loop header in front of the first request of the next stage, and the whole loop as a
sequence of waits, runs of load requests and stores; what stands behind the exec-mask branch of a half-trip (the row tail,
which waits for its own loads) is folded into "| tail |"."""
import re
import sys

def rows(path):
    s=open(path).read(); out={}
    for m in re.finditer(r'^(_ZN3spk1k17spmv_dict2_kernelI(\w+?)EEvNS0_8DictArgs\w+):\s', s, re.M):
        name=','.join(re.findall(r'L[bi](\d+)E', m.group(2)))
        if not name.endswith(',1'): continue
        lines=s[m.start(): s.index('.Lfunc_end', m.start())].split('\n')
        heads=[i for i,L in enumerate(lines) if re.match(r'^\.LBB\d+_\d+:.*=>This (Inner )?Loop Header: Depth=1',L)]
        best=None
        for h in heads:
            lab=lines[h].split(':')[0][1:].replace('LBB','BB')
            last=h
            for i in range(h+1,len(lines)):
                if re.match(r'^\.LBB',lines[i]) and ('Header='+lab) not in lines[i] and ('Parent Loop '+lab) not in lines[i]: break
                last=i
            n=sum('v_fma' in L for L in lines[h:last+1])
            if best is None or n>best[2]: best=(h,last,n)
        h,last,n=best
        seq=[]; depth2=False
        for i in range(h,last+1):
            L=lines[i].strip()
            if re.match(r'^\.LBB',L):
                depth2 = 'Depth=2' in L or 'Depth 2' in L
                continue
            if 's_waitcnt vmcnt' in L: seq.append(re.search(r'vmcnt\(\d+\)',L).group(0))
            elif re.search(r'(global|buffer)_load',L):
                if seq and seq[-1].startswith('load x'): seq[-1]='load x%d'%(int(seq[-1][6:])+1)
                else: seq.append('load x1')
            elif re.search(r'(global|buffer)_store',L): seq.append('store')
            elif 's_cbranch_exec' in L: seq.append('[exec branch]')
        hdr=[]
        for x in seq:
            if x.startswith('load'): break
            hdr.append(x)
        out[name]=(hdr,seq)
    return out
old,new=rows(sys.argv[1]),rows(sys.argv[2])
for k in sorted(new):
    print('spmv_dict2_kernel<%s>'%k)
    print('  header, before the first request of the next stage')
    print('    parent: s_waitcnt '+(', '.join(old[k][0]) or '(none)'))
    print('    now:    s_waitcnt '+(', '.join(new[k][0]) or '(none)'))
    for tag,r in (('parent',old[k]),('now',new[k])):
        # the pipelined part only: up to the first exec branch of each half (the row tail behind it waits for its own loads)
        s=[]; skip=False
        for x in r[1]:
            if x=='[exec branch]':
                if not skip: s.append('| tail |')
                skip=True; continue
            if x=='store': skip=False
            if not skip: s.append(x)
        print('  loop, %s: %s'%(tag,' '.join(s)))
    print()
