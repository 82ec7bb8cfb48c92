"""
Compare two register reports of the library (`make -C er3t_amd/csrc report 2> report.log`, -Rpass-analysis=kernel-resource-usage):
every kernel of the first report must be in the second with every printed figure identical; the kernels only the second one has are
listed with VGPR / scratch / waves per SIMD / SGPR spill.  (The fifth template argument of k_transport was a bool before the
solar+thermal source: Lb0E / Lb1E of an older report are read as Li0E / Li1E; the second one a bool and k_rays without its sixth argument
before the thermal cameras.  k_transport_lean has a sixth argument, the form of its entry records, and k_entry is a template over it since
the short entry records: the kernels of an older report are read as the long form's; k_bin_count / k_bin_scan / k_bin_scatter changed their
arguments with the per-block counts and are compared by their plain names.)

    python tools/resource_usage_diff.py parent_report.log new_report.log
"""
import re
import sys


def parse(fn):
    out, cur = {}, None
    for line in open(fn):
        m = re.search(r'remark: Function Name: (\S+)', line)
        if m:
            cur = m.group(1); out[cur] = []
            continue
        m = re.search(r'remark:\s+([A-Za-z \[\]/]+): (\S+) \[-Rpass', line)
        if m and cur:
            out[cur].append((m.group(1).strip(), m.group(2)))
    return out


def norm(name):
    name = re.sub(r'(k_transportILb\dELb\dELb\dELb\dE)Lb(\d)E', r'\1Li\2E', name)
    name = re.sub(r'(k_transportILb\dE)Lb(\d)E', r'\1Li\2E', name)                    # MARCH: a bool before the thermal cameras
    name = re.sub(r'(k_raysILb\dELb\dELb\dELb\dELb\dE)(E)', r'\1Lb0E\2', name)      # THERM: a sixth argument since then
    name = re.sub(r'(k_transport_leanILb\dELb\dELi\dELi\dELi\d+E)(E)', r'\1Li3E\2', name)   # EF: the long entry records
    name = re.sub(r'7k_entryENS_', '7k_entryILi3EEEvNS_', name)
    return re.sub(r'(_ZN4mi3d\d+k_bin_(?:count|scan|scatter))E.*', r'\1', name)


def main(parent, new):
    a = {norm(k): v for k, v in parse(parent).items()}
    b = {norm(k): v for k, v in parse(new).items()}
    bad = 0
    for k, v in a.items():
        if k not in b:
            print('MISSING', k); bad += 1
        elif b[k] != v:
            print('DIFF', k, [x for x in zip(v, b[k]) if x[0] != x[1]]); bad += 1
    print('%d kernels of the parent, %d differ; %d new kernels' % (len(a), bad, len(set(b) - set(a))))
    for k in sorted(set(b) - set(a)):
        d = dict(b[k])
        print(k, 'VGPR', d['VGPRs'], 'scratch', d['ScratchSize [bytes/lane]'], 'waves/SIMD', d['Occupancy [waves/SIMD]'], 'SGPR spill', d['SGPRs Spill'])
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(*sys.argv[1:3]))
