"""A pure-Python restatement of the decoding-step commit (include/iseg_hip.h, iseg_decode_commit): the state machine that replaces the tail of
sample_loop's body (iseg_amd/nlp/samplers.py) and the head of its next iteration.  Lists of ints and bools, no torch: the yardstick of the
kernel (tests/test_decode_graph_gpu.py) and, iterated, of sample_loop itself (tests/test_decode_graph_host.py)."""


class State:
    """prompt [B][S] ints, mask [B][S] bools (true = user token), pos: the index of the previous token, cur_ids [B], done [B] bools"""

    def __init__(self, prompt, mask, index, end_token_id=None):
        self.prompt = [list(map(int, row)) for row in prompt]
        self.mask = [list(map(bool, row)) for row in mask]
        self.B, self.S = len(self.prompt), len(self.prompt[0])
        self.pos = int(index) - 1
        self.end = -1 if end_token_id is None else int(end_token_id)
        self.cur_ids = [row[self.pos] if 0 <= self.pos < self.S else 0 for row in self.prompt]
        # the caller's initial done: ((prompt == end) & ~mask).any(-1)
        self.done = [self.end >= 0 and any(t == self.end and not m for t, m in zip(row, mrow)) for row, mrow in zip(self.prompt, self.mask)]

    def snapshot(self):
        return ([list(r) for r in self.prompt], self.pos, list(self.cur_ids), list(self.done))


def frozen(st):
    return not (0 <= st.pos + 1 < st.S) or (st.end >= 0 and all(st.done))


def commit(st, tokens):
    """one launch: tokens [B] is the sampler's choice -> True if the state advanced"""
    if frozen(st):
        return False
    col = st.pos + 1
    for b in range(st.B):
        user = st.mask[b][col]
        t = st.prompt[b][col] if user else int(tokens[b])
        st.prompt[b][col] = t
        st.cur_ids[b] = t
        if st.end >= 0 and t == st.end and not user:
            st.done[b] = True
    st.pos = col
    return True


def run(st, choose, extra=0):
    """iterate to the end (S - index launches, as generate_step replays) plus `extra` launches; choose(prompt, index) -> tokens [B] is the
    synthetic `next` + get_next_token, called only for steps that are live -> the number of live steps"""
    live = 0
    for _ in range(max(st.S - (st.pos + 1), 0) + extra):
        tokens = [0] * st.B if frozen(st) else choose(st.prompt, st.pos + 1)
        live += int(commit(st, tokens))
    return live
