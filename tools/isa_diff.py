#!/usr/bin/env python3
"""Is the device code of two csrc trees the same, kernel by kernel?  (compile time, no GPU)

    tools/isa_diff.py PARENT_CSRC NEW_CSRC [--extra=-DAMX_STATS] [--work DIR] [-j N] > report.txt

Every *.hip of both directories is compiled to gfx950 assembly with the FLAGS of that directory's Makefile
(+ --extra, + --cuda-device-only -S).  Functions are matched by demangled name, whatever unit they sit in, and two
things are compared: the instruction stream (comments dropped, local labels renumbered in order of appearance) and, for
kernels, the whole .amdhsa_kernel descriptor block.  Exit status 0: the same set of functions, none differing.
Assembly is kept under --work (default: a temporary directory) and compiled again only when a source of its tree is newer.
"""
import argparse, concurrent.futures, glob, os, re, subprocess, sys, tempfile


def makefile_flags(csrc):
    text = open(os.path.join(csrc, 'Makefile')).read()
    var = dict(re.findall(r'^(\w+)\s*\??=\s*(.*)$', text, re.M))
    return var['FLAGS'].replace('$(ARCH)', var.get('ARCH', 'gfx950')).split()


def assemble(csrc, out, extra, jobs):
    os.makedirs(out, exist_ok=True)
    flags = makefile_flags(csrc) + extra + ['--cuda-device-only', '-S']
    srcs = glob.glob(os.path.join(csrc, '*.h*')) + glob.glob(os.path.join(csrc, '../../include/*.h'))
    newest = max(os.path.getmtime(f) for f in srcs)
    todo = []
    for hip in sorted(glob.glob(os.path.join(csrc, '*.hip'))):
        s = os.path.join(out, os.path.basename(hip)[:-4] + '.s')
        if not (os.path.exists(s) and os.path.getmtime(s) > newest):
            todo.append(['/opt/rocm/bin/hipcc'] + flags + ['-o', s, hip])
    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        for cmd, r in zip(todo, ex.map(lambda c: subprocess.run(c, capture_output=True, text=True), todo)):
            if r.returncode:
                sys.exit('failed: %s\n%s' % (' '.join(cmd), r.stderr))
    for s in glob.glob(os.path.join(out, '*.s')):       # units that left the tree
        if not os.path.exists(os.path.join(csrc, os.path.basename(s)[:-2] + '.hip')):
            os.remove(s)


LABEL = re.compile(r'\.L(BB|func_end|func_begin|tmp)\d+(_\d+)?')


def functions(path):
    """{mangled name: (instructions, descriptor lines or None, resource comments)} of one assembly file"""
    lines = open(path).read().split('\n')
    types = set(re.findall(r'^\s*\.type\s+(\S+),@function', '\n'.join(lines), re.M))
    out, i = {}, 0
    while i < len(lines):
        m = re.match(r'^(\S+):', lines[i])
        if not (m and m.group(1) in types):
            i += 1
            continue
        # name: instructions [.section .rodata / .amdhsa_kernel ... .end_amdhsa_kernel / .text] .Lfunc_end<n>: ... ; Kernel info: ... .text | .section .text.<name>
        name, body, desc, seen, in_desc = m.group(1), [], None, {}, False
        i += 1
        while i < len(lines) and not re.match(r'^\.Lfunc_end\d+:', lines[i]):
            t = lines[i].split(';')[0].strip()
            if t.startswith('.amdhsa_kernel'):
                in_desc, desc = True, []
            if in_desc:
                desc.append(t)
                in_desc = not t.startswith('.end_amdhsa_kernel')
            elif t:
                body.append(LABEL.sub(lambda k: seen.setdefault(k.group(0), '.L%d' % len(seen)), t))
            i += 1
        res = {}
        while i < len(lines) and not re.match(r'^\t(\.text|\.section\t\.text)', lines[i]):
            k = re.match(r'^; (TotalNumSgprs|NumVgprs|NumAgprs|ScratchSize|LDSByteSize): (\d+)', lines[i])
            if k:
                res[k.group(1)] = int(k.group(2))
            i += 1
        out[name] = (body, desc, res)
    return out


def tree(asm_dir):
    mangled = {}
    for s in sorted(glob.glob(os.path.join(asm_dir, '*.s'))):
        for n, v in functions(s).items():
            mangled.setdefault(n, []).append((os.path.basename(s)[:-2], v))
    names = sorted(mangled)
    dem = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True, check=True).stdout.split('\n')
    out = {}
    for n, d in zip(names, dem):
        if len(mangled[n]) > 1 and any(v != mangled[n][0][1] for _, v in mangled[n]):
            # the same name in several units (anonymous namespaces, helpers that were not inlined): keep them apart
            for u, v in mangled[n]:
                out['%s [%s]' % (d, u)] = (u, v)
        else:
            out[d] = ('+'.join(u for u, _ in mangled[n]), mangled[n][0][1])      # (the same code in several units: all of them named)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('parent'), ap.add_argument('new')
    ap.add_argument('--extra', action='append', default=[])
    ap.add_argument('--work', default=None)
    ap.add_argument('-j', type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    work = a.work or tempfile.mkdtemp(prefix='isa_diff_')
    tag = ''.join(re.sub(r'\W', '', e) for e in a.extra) or 'plain'
    da, db = os.path.join(work, 'parent_' + tag), os.path.join(work, 'new_' + tag)
    assemble(a.parent, da, a.extra, a.j)
    assemble(a.new, db, a.extra, a.j)
    A, B = tree(da), tree(db)
    print('# device code, parent against new tree, flags: %s' % ' '.join(makefile_flags(a.new) + a.extra))
    print('# kernels of the parent: %d of %d functions; of the new tree: %d of %d' % (
        sum(1 for v in A.values() if v[1][1] is not None), len(A), sum(1 for v in B.values() if v[1][1] is not None), len(B)))
    print('# name | unit (parent -> new) | instructions | VGPRs AGPRs SGPRs | scratch bytes | static LDS bytes | verdict')
    bad = 0
    for n in sorted(set(A) | set(B)):
        if n not in A or n not in B:
            print('%s | only in the %s tree' % (n, 'parent' if n in A else 'new'))
            bad += 1
            continue
        (ua, (ia, ka, ra)), (ub, (ib, kb, rb)) = A[n], B[n]
        same = ia == ib and ka == kb and ra == rb
        bad += not same
        what = 'identical' if same else 'DIFFERS (%s)' % ', '.join(w for w, d in (('instructions', ia != ib), ('descriptor', ka != kb), ('resources', ra != rb)) if d)
        print('%s | %s | %d | %d %d %d | %d | %d | %s' % (n, ua if ua == ub else ua + ' -> ' + ub, len([t for t in ib if not t.endswith(':') and not t.startswith('.')]),
              rb.get('NumVgprs', 0), rb.get('NumAgprs', 0), rb.get('TotalNumSgprs', 0), rb.get('ScratchSize', 0), rb.get('LDSByteSize', 0), what))
    print('# %d functions compared, %d differing or unmatched' % (len(set(A) | set(B)), bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
