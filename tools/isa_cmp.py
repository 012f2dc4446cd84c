"""Static comparison of two builds of the kernel units, kernel by kernel.

usage: python tools/isa_cmp.py before.s before_resource.txt after.s after_resource.txt [four more per unit ...]

The .s files are `make asm` outputs (build/<unit>.s), the resource files
`make resource` outputs -- of the one unit or of all of them, kernels are
found by name.  One report per group of four, headed `== <unit>` when there
are several.  Per kernel of the step / rollout / render / policy families:
the instruction total and its valu / salu / lds / vmem split
(tools/isa_segs.py's classes), VGPRs, SGPRs, occupancy, LDS size and scratch
size, before -> after, and whether the instruction streams are equal as text
(comments, directives and labels stripped, label references renumbered
away).  Every other kernel is checked for an equal stream and equal
resources.  The last lines state the conditions a refactor has to meet, for
every kernel: it exists on both sides (a unit that gained or lost an
instantiation shows up), scratch stays 0, occupancy does not drop, LDS size
is unchanged.  The exit status is 1 if any group violates one.
"""
import collections
import re
import subprocess
import sys

FAMILIES = ('k_step', 'k_rollout2', 'k_rollout', 'k_render', 'k_policy_greedy')
KEYS = ('VGPRs', 'TotalSGPRs', 'Occupancy', 'LDS', 'ScratchSize')


def kernels(path):
    s = open(path).read()
    out = {}
    for m in re.finditer(r'^(_Z\w+):', s, re.M):
        j = s.find('.Lfunc_end', m.start())
        if j < 0:
            continue
        body = []
        for l in s[m.start():j].split('\n')[1:]:
            l = l.split(';')[0].strip()
            if l and not l.startswith('.') and not l.endswith(':'):
                body.append(re.sub(r'\.LBB\d+_\d+', '.L', l))
        out[m.group(1)] = body
    return out


def kind(op):
    if op.startswith('v_'):
        return 'valu'
    if op.startswith('s_'):
        return 'salu'
    if op.startswith('ds_'):
        return 'lds'
    if op.startswith(('global', 'buffer', 'flat')):
        return 'vmem'
    return 'other'


def mix(body):
    c = collections.Counter(kind(l.split()[0]) for l in body)
    return len(body), c['valu'], c['salu'], c['lds'], c['vmem']


def resources(path):
    out, cur = {}, None
    for l in open(path):
        m = re.search(r'Function Name: (\S+)', l)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r'\b(VGPRs|TotalSGPRs|Occupancy|LDS Size|ScratchSize)[^:]*: (\d+)', l)
        if m and cur is not None:
            cur.setdefault(m.group(1).split()[0], int(m.group(2)))
    return out


def demangle(names):
    r = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, r.stdout.split('\n')))


def short_name(full):
    return re.sub(r'\(.*$', '', re.sub(r'^(void )?st::\(anonymous namespace\)::', '', full))


def main(pa, pr, na, nr):
    ka, kb, ra, rb = kernels(pa), kernels(na), resources(pr), resources(nr)
    names = [n for n in ka if n in ra]
    added = [n for n in kb if n in rb and n not in names]
    dm = demangle(names + added)
    bad, same_n, diff_n, other_same, other_diff, res_diff = [], 0, 0, 0, [], []
    only = ['%s (before only)' % short_name(dm[n]) for n in names if n not in kb or n not in rb]
    only += ['%s (after only)' % short_name(dm[n]) for n in added]
    print('kernel | instructions: total valu/salu/lds/vmem, before -> after | '
          'VGPRs SGPRs occupancy LDS scratch, before -> after | stream')
    for n in names:
        short = short_name(dm[n])
        if n not in kb or n not in rb:
            continue
        same = ka[n] == kb[n]
        x, y = ra[n], rb[n]
        if any(x.get(k) != y.get(k) for k in KEYS):
            res_diff.append(short)
        if x.get('ScratchSize') == 0 and y.get('ScratchSize') != 0:
            bad.append(short + ' scratch')
        if y.get('Occupancy', 0) < x.get('Occupancy', 0):
            bad.append(short + ' occupancy')
        if y.get('LDS') != x.get('LDS'):
            bad.append(short + ' LDS size')
        if short.split('<')[0] not in FAMILIES:
            other_same += same
            if not same:
                other_diff.append(short)
            continue
        same_n += same
        diff_n += not same
        print('%s | %d %d/%d/%d/%d -> %d %d/%d/%d/%d | %s -> %s | %s' % (
            (short,) + mix(ka[n]) + mix(kb[n]) + (' '.join(str(x.get(k)) for k in KEYS),
                                                ' '.join(str(y.get(k)) for k in KEYS),
                                                'identical' if same else 'differs')))
    print('listed kernels: %d identical streams, %d differ' % (same_n, diff_n))
    print('other kernels: %d identical streams, %d differ%s' % (
        other_same, len(other_diff), ': ' + ', '.join(other_diff) if other_diff else ''))
    print('VGPRs, SGPRs, occupancy, LDS size, scratch of every kernel: %s' % (
        'equal' if not res_diff else 'differ for ' + ', '.join(res_diff)))
    bad = only + bad
    print('kernels on one side only: %s' % (', '.join(only) if only else 'none'))
    print('no kernel on one side only, scratch stays 0, occupancy does not drop, LDS size unchanged: %s' % (
        'all hold' if not bad else 'VIOLATED: ' + ', '.join(bad)))
    return 1 if bad else 0


if __name__ == '__main__':
    args = sys.argv[1:]
    if not args or len(args) % 4:
        sys.exit(__doc__)
    status = 0
    for i in range(0, len(args), 4):
        if len(args) > 4:
            print('== ' + re.sub(r'^.*/|\.s$', '', args[i + 2]))
        status |= main(*args[i:i + 4])
    sys.exit(status)
