"""Per-kernel ISA statistics of a gfx950 assembly file (hipcc --save-temps=obj, or
--cuda-device-only -S): global loads (and how many use SGPR-base addressing), VALU count, VGPRs,
scratch, and a digest of the kernel's instruction text with the local label numbers normalised
(equal digests of two builds: the same instructions).  A template instance prints with its
arguments, k_scalars<OptGeneric, Budget>."""
import hashlib
import re
import sys


def instance(sym):
    """k_name<args> of a mangled kernel symbol: the namespace's types, float / double, bool and int literals and
    packs, which is what the kernels here are instantiated on; anything else prints as '?'."""
    m = re.search(r'(\d+)(k_[a-z0-9_]+)', sym)
    if not m or int(m.group(1)) != len(m.group(2)):
        return sym
    rest, args, depth = sym[m.end():], [], 0
    if not rest.startswith('I'):
        return m.group(2)
    rest = rest[1:]
    while rest:
        if rest[0] == 'J':                       # a pack: its elements join the list
            depth, rest = depth + 1, rest[1:]
        elif rest[0] == 'E':
            if depth == 0:
                break
            depth, rest = depth - 1, rest[1:]
        elif (a := re.match(r'NS_(\d+)', rest)):
            n = int(a.group(1))
            args.append(rest[a.end():a.end() + n])
            rest = rest[a.end() + n + 1:]        # the name and the E that closes the nested name
        elif (a := re.match(r'Lb([01])E', rest)):
            args.append('true' if a.group(1) == '1' else 'false')
            rest = rest[a.end():]
        elif (a := re.match(r'Li(n?)(\d+)E', rest)):
            args.append(('-' if a.group(1) else '') + a.group(2))
            rest = rest[a.end():]
        elif rest[0] in 'fd':                    # a builtin type argument: float, double
            args.append('float' if rest[0] == 'f' else 'double')
            rest = rest[1:]
        else:
            args.append('?')
            break
    return f"{m.group(2)}<{', '.join(args)}>"


def text_digest(body):
    """sha1 of the instruction lines up to the kernel's end, comments and directives dropped"""
    lines = []
    for ln in body.split('\n')[1:]:
        ln = ln.split(';')[0].strip()
        if ln.startswith('.Lfunc_end'):
            break
        if not ln or (ln.startswith('.') and not ln.startswith('.LBB')):
            continue
        lines.append(re.sub(r'\.LBB\d+_', '.LBB_', ln))
    return hashlib.sha1('\n'.join(lines).encode()).hexdigest()[:12]


s = open(sys.argv[1]).read()
labels = [(m.start(), m.group(1)) for m in re.finditer(r'^(_Z\w+):', s, re.M)]
for n, (pos, name) in enumerate(labels):
    end = labels[n + 1][0] if n + 1 < len(labels) else len(s)
    body = s[pos:end]
    gl = len(re.findall(r'^\s+global_load', body, re.M))
    sad = len(re.findall(r'^\s+global_load\S* v\S+, v\d+, s\[', body, re.M))
    va = len(re.findall(r'^\s+v_', body, re.M))
    nv = re.search(r'NumVgprs:\s+(\d+)', body)
    sc = re.search(r'ScratchSize:\s+(\d+)', body)
    print(f"{instance(name):42s} gload={gl:4d} saddr={sad:4d} valu={va:5d} "
          f"vgpr={nv.group(1) if nv else '?':>4s} scratch={sc.group(1) if sc else '?'} text={text_digest(body) if nv else '-'}")
