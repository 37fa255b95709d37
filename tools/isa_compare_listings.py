"""Is the device code of two trees the same? Compares two directories of `hipcc -S --cuda-device-only` listings (the FLAGS of
csrc/Makefile), one per kernel_*.hip, function by function: the body, the kernel descriptor and the resource lines behind it
(.set ...num_vgpr / scratch / LDS sizes) — the order in which template instantiations are emitted follows the host code's order
of use and is ignored, basic-block label numbers are normalised, lines that only carry source paths, line numbers or the
per-compilation id (__hip_cuid_*, a hash of the source text) are dropped.

    python tools/isa_compare_listings.py old_dir/ new_dir/ [--mask-argument-offsets] [--all]

--all: every differing line of every differing function (default: the first three of each, for three functions per file).

--mask-argument-offsets: for a change that moves fields inside a kernel's argument block or inside A1Plan and nothing else.
Masks the immediate offset of scalar and global loads whose base register pair holds the kernel-argument pointer or the plan
pointer, and the descriptor's / metadata's kernel-argument sizes and offsets; everything else must still be identical. Which
pairs hold those pointers is followed along the listing, top to bottom: s[0:1] at entry (the kernel-argument segment pointer),
s_mov copies of it and spills to a lane (v_writelane / v_readlane), and — in a kernel whose first parameter is `const A1Plan*` — the pair loaded from argument offset 0. A
register stops counting when a scalar instruction overwrites it. Addresses formed another way (argument pointer + literal in an
s_add_u32, say) are not masked: they show up as differences, to be read and explained.
"""
import re,sys,os
args=[a for a in sys.argv[1:] if not a.startswith('--')]
mask='--mask-argument-offsets' in sys.argv
every='--all' in sys.argv
old,new=args[:2]
def regs(op):
    """scalar registers an operand names: s5 -> {5}, s[4:7] -> {4..7}"""
    m=re.fullmatch(r's\[(\d+):(\d+)\]',op)
    if m: return set(range(int(m.group(1)),int(m.group(2))+1))
    m=re.fullmatch(r's(\d+)',op)
    return {int(m.group(1))} if m else set()
def masked(sym,lines):
    role={0:('arg',0),1:('arg',1)}  # scalar register -> which pointer it holds, low / high half
    def held(op):
        r=sorted(regs(op))
        return role[r[0]][0] if len(r)==2 and r[0] in role and r[1] in role and role[r[0]][0]==role[r[1]][0] and (role[r[0]][1],role[r[1]][1])==(0,1) else None
    takes_plan='PKNS_6A1PlanE' in sym  # (mangled) its first parameter: const A1Plan*
    out,spilled=[],{}
    for l in lines:
        m=re.match(r'\t(\w+)\s+([^;]*)',l)
        if not m or l.startswith('\t.'):
            if re.match(r'\t\t\.amdhsa_kernarg_size ',l): l='\t\t.amdhsa_kernarg_size <masked>'
            out.append(l); continue
        op,ops=m.group(1),[o.strip() for o in m.group(2).split(',')]
        base=None
        if op.startswith('s_load_') and len(ops)>=3: base=ops[1]
        elif op.startswith('global_load_'): base=next((o.split()[0] for o in ops[1:] if o.startswith('s[')),None)
        gets={}  # roles this instruction's result takes
        if base and held(base):
            if takes_plan and held(base)=='arg' and op.startswith('s_load_dwordx') and ops[2]=='0x0': gets=dict(zip(sorted(regs(ops[0])),(('plan',0),('plan',1))))
            l=re.sub(r'(, )0x[0-9a-f]+\s*$',r'\1<imm>',re.sub(r'offset:\d+','offset:<imm>',l))
        elif op=='v_writelane_b32' and regs(ops[1]):  # a spill to a lane, and back
            spilled[ops[0],ops[2]]=role.get(min(regs(ops[1])))
        elif op=='v_readlane_b32' and regs(ops[0]):
            role.pop(min(regs(ops[0])),None)
            if spilled.get((ops[1],ops[2])): role[min(regs(ops[0]))]=spilled[ops[1],ops[2]]
        elif op in ('s_mov_b32','s_mov_b64') and len(ops)==2:
            gets={d:role[r] for d,r in zip(sorted(regs(ops[0])),sorted(regs(ops[1]))) if r in role}
        if op.startswith('s_') and not op.startswith(('s_cmp','s_cbranch','s_branch','s_waitcnt','s_barrier','s_nop','s_sleep','s_endpgm','s_setprio','s_bitcmp')):
            for r in regs(ops[0]): role.pop(r,None)  # a scalar write ends what the register held
            role.update(gets)
        out.append(l)
    return out
def split(path):
    """symbol -> text of its function (body, kernel descriptor, resource lines), normalised; plus the rest of the file"""
    funcs,rest,cur={},[],None
    for l in open(path):
        t=l.strip()
        if t.startswith(('.file','.loc','.ident')) or '__hip_cuid_' in l:
            continue  # source paths / line numbers / the per-compilation id derived from the source text
        m=re.match(r'\t\.section\t\.text\.(_Z\w+),',l) or re.match(r'\t\.amdhsa_kernel (_Z\w+)',l)
        if m: cur=m.group(1); funcs.setdefault(cur,[])  # (the section is entered again behind the descriptor)
        elif re.match(r'\t\.(text|amdgpu_metadata)',l) or (l.startswith('\t.section') and '.rodata' not in l): cur=None
        l=re.sub(r'\.L(BB|func_begin|func_end|tmp)\d+(_\d+)?',lambda m:'.L'+m.group(1)+(m.group(2) or ''),l.rstrip('\n'))
        if mask and cur is None: l=re.sub(r'^(\s+(- )?\.(kernarg_segment_size|size|offset):\s+)\d+',r'\1<masked>',l)
        (funcs[cur] if cur else rest).append(l)
    if mask: funcs={k:masked(k,v) for k,v in funcs.items()}
    return funcs,rest
def resources(lines):
    """instruction count and the resource lines of a function"""
    n=sum(1 for l in lines if re.match(r'\t[a-z]\w+',l) and not l.startswith('\t.'))
    r={m.group(1):m.group(2) for l in lines for m in [re.match(r'\t\.set \S+\.(num_vgpr|num_agpr|numbered_sgpr|private_seg_size), (\d+)',l) or re.match(r'\t\t\.amdhsa_(group_segment_fixed_size) (\d+)',l)] if m}
    return n,r
for f in sorted(os.listdir(old)):
    if not f.endswith('.s'): continue
    fa,ra=split(os.path.join(old,f)); fb,rb=split(os.path.join(new,f))
    la=sorted(re.findall(r'^(_Z\w+):',open(os.path.join(old,f)).read(),re.M)); lb=sorted(re.findall(r'^(_Z\w+):',open(os.path.join(new,f)).read(),re.M))
    diff=[k for k in fa if fa[k]!=fb.get(k)]
    res=[k for k in fa if k in fb and resources(fa[k])!=resources(fb[k])]
    print(f"{f}: symbol labels {len(la)} / {len(lb)}, {'same set' if la==lb else 'SETS DIFFER'}; functions {len(fa)} / {len(fb)}, "
          f"{len(fa)-len(diff)} identical, {len(diff)} different; instruction counts, registers, LDS, scratch: {'same in all' if not res else 'DIFFER in '+str(len(res))}; "
          f"same order: {list(fa)==list(fb)}; rest of file (sorted lines) {'identical' if sorted(ra)==sorted(rb) else 'DIFFERENT'}")
    for k in diff if every else diff[:3]:
        x,y=fa[k],fb.get(k,[])
        pairs=[(p,q) for p,q in zip(x,y) if p!=q]
        print('   ',k,len(x),len(y),pairs if every else pairs[:3])
