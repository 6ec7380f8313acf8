"""The transducer beam search of liteasr/models/transducer.py:137-206, restated with lists of
Python objects (test oracle; the product path is liteasr_amd/decoding.py on csrc/rnnt_search.hip).

Per encoder frame: A = kept, B = []; ten times pop the first best-scoring hypothesis of A,
run the prediction-network step of its last token (memoised by the whole yseq), take the
log-prob row, append to A the 10 best non-blank tokens in descending order (score + logp,
the post-step state, yseq + [k]) and to B the same hypothesis with score + logp[0] and its
state unchanged; then kept = B.  Scores are Python floats.  The result is the first
hypothesis of kept that maximises score / len(yseq).  No prefix merging: hypotheses with the
same yseq stay separate and share only the memoised step (here: the trie node).

The arithmetic is the caller's:
  step(node) -> state     the state after feeding node.token from node.parent.state (the
                          root's parent is None: zero state)
  logp(frame, node) -> V floats, the log-softmax row of frame ``frame`` for node.state
"""

BEAM = 10


class Node:
    """One distinct yseq."""

    def __init__(self, parent, token):
        self.parent, self.token = parent, token
        self.yseq = (parent.yseq if parent is not None else ()) + (token,)
        self.state = None
        self.children = {}

    def child(self, token):
        n = self.children.get(token)
        if n is None:
            n = self.children[token] = Node(self, token)
        return n


def beam_search(frames, step, logp, trace=None):
    """Returns (yseq list, best score / len, number of executed steps).  trace (a list)
    receives (yseq tuple, score, len(A) at the pop) per expansion."""
    root = Node(None, 0)
    if frames <= 0:
        return [0], 0.0, 0
    kept = [(root, 0.0)]
    steps = 0
    for t in range(frames):
        A, B = kept, []
        while len(B) < BEAM:
            i = max(range(len(A)), key=lambda j: A[j][1])  # first maximum in list order
            if trace is not None:
                trace.append((A[i][0].yseq, A[i][1], len(A)))
            node, score = A.pop(i)
            if node.state is None:
                node.state = step(node)
                steps += 1
            row = [float(v) for v in logp(t, node)]
            top = sorted(range(1, len(row)), key=lambda k: (-row[k], k))[:BEAM]
            for k in top:
                A.append((node.child(k), score + row[k]))
            B.append((node, score + row[0]))
        kept = B
    norm = [s / len(n.yseq) for n, s in kept]
    b = max(range(len(kept)), key=lambda j: norm[j])
    return list(kept[b][0].yseq), norm[b], steps
