#!/usr/bin/env python3
"""Development: which product of learn_stepsize's two weighted sums did the compiler fuse, in every function that holds the rule?

    python scripts/dev/fused_products.py build/variants/libpotus_parent.so us_potus_model_amd/libpotus_hmc.so

(1 - eta) s_bar + eta (delta - as) and (1 - x_eta) x_bar + x_eta x can each become fma(first product) or fma(second product); the two
differ by an ulp now and then, and with them every later draw.  For every `v_add_f64 X, -Y, 1.0` of the functions below this prints
where Y came from (`eta`: a division with numerator 1.0) and the first instruction that reads X: `v_fmac` / `v_fma` = the product with
1 - Y is the fused one, `v_mul` = the other one is.  Two builds give the same step sizes only if these agree function by function."""
import re, sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent))
from same_device_code import functions
KEYS = ('k_dn_end', 'cold_transition_end', 'cold_twin1_end', 'cl_cold_transition_end', 'cl_cold_twin_end')
def regs(tok):
    m = re.match(r'-?\|?v\[(\d+):(\d+)\]', tok)
    return set(range(int(m.group(1)), int(m.group(2)) + 1)) if m else set()
def classify(buf):
    out = []
    for i, ins in enumerate(buf):
        m = re.match(r'v_add_f64 (v\[\d+:\d+\]), -(v\[\d+:\d+\]), 1\.0$', ins)
        if not m: continue
        X = regs(m.group(1)); src = m.group(2)
        # where does the subtracted value come from: a division with numerator 1.0 (eta) or not (x_eta)
        origin = '?'
        for j in range(i - 1, max(i - 400, 0), -1):
            ops = buf[j].split(None, 1)
            if len(ops) > 1 and regs(ops[1].split(',')[0].strip()) == regs(src):
                origin = 'eta' if buf[j].startswith('v_div_fixup_f64') and buf[j].rstrip().endswith('1.0') else buf[j].split()[0]
                break
        use = 'unused'
        for j in range(i + 1, min(i + 400, len(buf))):
            ops = buf[j].split(None, 1)
            if len(ops) < 2: continue
            toks = [t.strip() for t in ops[1].split(',')]
            if any(regs(t) == X for t in toks[1:]):
                use = ops[0]; break
            if regs(toks[0]) & X: use = 'overwritten'; break
        out.append((origin, use))
    return out
for lib in sys.argv[1:]:
    f = functions(lib)
    print('==', lib)
    for n in sorted(f):
        if any(k in n for k in KEYS):
            print('  %-40s %s' % (n[:40], [c for c in classify(f[n]) if c[0] == 'eta' or 'fma' in c[1] or 'mul' in c[1]]))
