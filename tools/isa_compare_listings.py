"""Is the device code of two trees the same? Compares two directories of `hipcc -S --cuda-device-only` listings (the FLAGS of
csrc/Makefile), one per kernel_*.hip, function section by function section — the order in which template instantiations are
emitted follows the host code's order of use and is ignored, basic-block label numbers are normalised, lines that only carry
source paths, line numbers or the per-compilation id (__hip_cuid_*, a hash of the source text) are dropped.

    python tools/isa_compare_listings.py old_dir/ new_dir/
"""
import re,sys,os
old,new=sys.argv[1:3]
def split(path):
    """symbol -> text of its section (function body + kernel descriptor), normalised; plus the rest of the file"""
    funcs,rest,cur={},[],None
    for l in open(path):
        t=l.strip()
        if t.startswith(('.file','.loc','.ident')) or '__hip_cuid_' in l:
            continue  # source paths / line numbers / the per-compilation id derived from the source text
        m=re.match(r'\t\.section\t\.text\.(_Z\w+),',l)
        if m: cur=m.group(1); funcs[cur]=[]
        elif re.match(r'\t\.(section|text|rodata|amdgpu_metadata)',l) or l.startswith('\t.section'): cur=None
        l=re.sub(r'\.L(BB|func_begin|func_end|tmp)\d+(_\d+)?',lambda m:'.L'+m.group(1)+(m.group(2) or ''),l.rstrip('\n'))
        (funcs[cur] if cur else rest).append(l)
    return funcs,rest
for f in sorted(os.listdir(old)):
    if not f.endswith('.s'): continue
    fa,ra=split(os.path.join(old,f)); fb,rb=split(os.path.join(new,f))
    la=sorted(re.findall(r'^(_Z\w+):',open(os.path.join(old,f)).read(),re.M)); lb=sorted(re.findall(r'^(_Z\w+):',open(os.path.join(new,f)).read(),re.M))
    diff=[k for k in fa if fa[k]!=fb.get(k)]
    print(f"{f}: symbol labels {len(la)} / {len(lb)}, {'same set' if la==lb else 'SETS DIFFER'}; function sections {len(fa)} / {len(fb)}, "
          f"{len(fa)-len(diff)} identical, {len(diff)} different; same order: {list(fa)==list(fb)}; rest of file (sorted lines) {'identical' if sorted(ra)==sorted(rb) else 'DIFFERENT'}")
    for k in diff[:3]:
        x,y=fa[k],fb.get(k,[])
        print('   ',k,len(x),len(y),[ (p,q) for p,q in zip(x,y) if p!=q][:3])
