"""The draft-size distribution that the exact-row verify forward is built on (LlamaRunner.ROWS_EXACT, profiles/rows_exact.md), pinned on
the CPU oracle: the reference's draft rule (max_predicts 60, alpha 4, K 8, len_bias 0) on bench.py's own request process puts three
quarters of its steps at drafts of exactly 5 nodes and one in six at exactly 9.  Should a later change of the workload's shape move the
drafts elsewhere, this fails and says that the 5- and 9-row forms no longer cover the steps they were instantiated for."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from oracle import sam_oracle as O  # noqa: E402


def test_three_quarters_of_the_headline_steps_draft_5_nodes_and_a_sixth_9():
    flat, off, docs = bench.synth_corpus(1 << 20)
    st = O.StaticSAM()
    fa, fp = O._i32(flat)
    oa, op = O._i64(off)
    O.lib().osam_add_batch(st._h, fp, op, len(off) - 1, bench.EOS)
    st.init_topk_next()
    dm = O.DraftModel(60, 4.0, 8, 0, sam_static=st)
    rng = np.random.default_rng(1000)
    sizes, steps, tokens = {}, 0, 0
    for _ in range(6):                                   # bench.cpu_baseline's loop, six requests
        prompt, target = bench.synth_request(rng, docs)
        dm.reset()
        dm.update(prompt)
        pos = len(prompt)
        while pos < len(prompt) + 512 and pos + 70 < len(target):
            ty, tok, anc = dm.lookup_raw(target[pos])
            n = len(tok)
            sizes[n] = sizes.get(n, 0) + 1
            depth, ok, best = [0] * n, [True] * n, 0
            for i in range(1, n):
                depth[i] = depth[anc[i]] + 1
                ok[i] = ok[anc[i]] and tok[i] == target[pos + depth[i]]
                if ok[i] and depth[i] > depth[best]:
                    best = i
            acc = target[pos:pos + depth[best] + 1]
            dm.update(acc)
            pos += len(acc)
            steps += 1
            tokens += len(acc)
    share = {n: c / steps for n, c in sorted(sizes.items())}
    print(f"{steps} steps, mean accept {tokens / steps:.3f}, draft sizes {({n: round(s, 3) for n, s in share.items()})}")
    assert steps > 1000
    assert share.get(5, 0.0) >= 0.60, share              # the reference gives 74.7 % on these inputs
    assert share.get(9, 0.0) >= 0.10, share              # ... and 15.7 %
