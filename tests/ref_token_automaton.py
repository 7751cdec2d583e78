"""numpy restatement of the token automaton (include/mila_cdna4.h: token automaton; Mila/TokenAutomaton.h): the state step, the effective table of a state and the
dead-end check, plus the random automata the tests share.  Nothing here calls the code under test."""
import numpy as np

FORBIDDEN = 0xFFFF
NEG_INF = np.float32(-np.inf)


def step(class_of, next_table, state, token):
    """the next state; a forbidden token leaves the state"""
    n = int(next_table[state, class_of[token]])
    return state if n == FORBIDDEN else n


def mask(class_of, next_table, state, base=None):
    """eff[i] = base[i] where next[state, class_of[i]] is not FORBIDDEN, else -inf (base None: zeros); float32, the base bits kept"""
    base = np.zeros(class_of.size, dtype=np.float32) if base is None else np.asarray(base, dtype=np.float32)
    return np.where(next_table[state, class_of] != FORBIDDEN, base, NEG_INF).astype(np.float32)


def dead_end(class_of, next_table, start, bias=None):
    """the first state, in breadth-first order from start, that keeps no token with a transition and a finite bias (bias None: all finite); None when there is
    none.  Reachability runs over such tokens only.  Per token, not per class: the slow, obvious form."""
    finite = np.ones(class_of.size, dtype=bool) if bias is None else np.isfinite(bias)
    seen, queue = {start}, [start]
    while queue:
        s = queue.pop(0)
        nxt = next_table[s, class_of].astype(np.int64)
        ok = (nxt != FORBIDDEN) & finite
        if not ok.any():
            return s
        for n in dict.fromkeys(nxt[ok].tolist()):      # in token order: the order the class form visits first-seen classes may differ, the SET of dead ends does not
            if n not in seen:
                seen.add(n)
                queue.append(n)
    return None


def random_automaton(vocab, num_states, num_classes, seed, forbid=0.5):
    """(class_of uint16 [vocab], next uint16 [S, C]): every class used when vocab allows, every state keeps at least one allowed class"""
    rng = np.random.default_rng(seed)
    class_of = rng.integers(0, num_classes, size=vocab).astype(np.uint16)
    if vocab >= num_classes:
        class_of[rng.permutation(vocab)[:num_classes]] = np.arange(num_classes, dtype=np.uint16)
    nxt = rng.integers(0, num_states, size=(num_states, num_classes)).astype(np.uint16)
    nxt[rng.random((num_states, num_classes)) < forbid] = FORBIDDEN
    present = np.unique(class_of)
    for s in range(num_states):
        if (nxt[s, present] == FORBIDDEN).all():
            nxt[s, present[rng.integers(len(present))]] = rng.integers(0, num_states)
    return class_of, nxt


def base_table(vocab, seed):
    """a base table with finite values of both signs, signed zeros and -inf entries"""
    rng = np.random.default_rng(seed)
    b = (rng.standard_normal(vocab) * 4.0).astype(np.float32)
    b[rng.random(vocab) < 0.2] = NEG_INF
    b[rng.random(vocab) < 0.05] = np.float32(-0.0)
    return b
