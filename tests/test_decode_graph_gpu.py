"""The decode step replayed from one captured HIP graph (GemmaCausalLM.compile(graph_decode=True)): the launchers that read the position from device
memory (iseg_gemma_rope_cache_at, iseg_gemma_decode_attention_at) bit for bit against the host-position launchers, one capture replayed at
several positions, their guard bands and what an out-of-range position leaves untouched, the commit kernel (iseg_decode_commit) against the
Python state machine of tests/decode_commit_ref.py, and the generation itself: token for token the eager loop's."""
import pytest
import torch

from tests import decode_commit_ref as R
from tests import guarded_memory as GM
from tests.test_gemma_cache_gpu import B, CASES, PROMPTS, S, _bits, _model, _prompts, bf16  # noqa: F401  (bf16 is a fixture)
from tests.test_kernels_gpu import DTYPES, rnd

pytestmark = pytest.mark.gpu

BORDERS = (0, 62, 63, 64, 65, 127, 128, 129)      # on and beside every border of the 64-key tiles, and S - Tn


def _pos(value):
    return torch.tensor([value], dtype=torch.int32, device="cuda")


# ---- decode attention: bit identity with the host-position launcher ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=["x".join(map(str, c[:2] + c[4:7])) for c in CASES])
def test_decode_attention_at_is_the_host_position_launcher_bit_for_bit(cuda, bf16, case):
    """shapes of tests/test_gemma_cache_gpu.py::CASES; every position on and beside a tile border and the last; Tn = 1 and, where 2 g <= 16 and
    the cache has two rows, Tn = 2; splits = 0 (the plan, which changes with the position), 3 and 1000 (clipped to the visible tiles).  The cache
    past the last visible key is NaN, so a key loaded from there shows."""
    from iseg_amd import kernels as K

    Bc, Sc, _, _, nq, nkv, h, _ = case
    cache0 = rnd((Bc, 2, Sc, nkv, h), 2).to(torch.bfloat16).cuda()
    pos_d = _pos(0)
    scale = float(h) ** -0.5
    checked = 0
    for Tn in (1, 2):
        if Tn > Sc or (nq // nkv) * Tn > 16:
            continue
        q = rnd((Bc, Tn, nq * h), 1).to(torch.bfloat16).cuda()
        for pos0 in sorted({p for p in BORDERS + (Sc - Tn,) if p + Tn <= Sc}):
            cache = cache0.clone()
            cache[:, :, pos0 + Tn:] = float("nan")
            pos_d.fill_(pos0)
            for splits in (0, 3, 1000):
                want = K.gemma_decode_attention(q, cache, pos0, nq, nkv, h, scale, splits)
                got = K.gemma_decode_attention_at(q, cache, pos_d, nq, nkv, h, scale, splits)
                assert torch.isfinite(want.float()).all()
                assert torch.equal(_bits(got), _bits(want)), (Tn, pos0, splits)
                checked += 1
    assert checked >= 3


# ---- rotary embedding into the cache -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("pos0", [300, 0])
def test_rope_cache_at_is_the_host_position_launcher_bit_for_bit(cuda, dtype, pos0):
    """the shape of test_rope_cache_at_position_300: q, the written rows and every other cache row (a poison pattern) carry the same bits"""
    from iseg_amd import functional as F
    from iseg_amd import nn

    Bc, Sc, Tn, nq, nkv, h = 2, 310, 3, 2, 1, 64
    nn.set_compute_dtype(dtype)
    try:
        x = rnd((Bc, Tn, (nq + 2 * nkv) * h), 5).to(dtype).cuda()
        pattern = 0x7FA5 if dtype == torch.bfloat16 else 0x7FA5A5A5
        caches = [torch.empty((Bc, 2, Sc, nkv, h), dtype=dtype, device="cuda") for _ in range(2)]
        for c in caches:
            _bits(c).fill_(pattern)
        want = F.gemma_rope_cache(x, caches[0], pos0, nq, nkv, h)
        got = F.gemma_rope_cache(x, caches[1], _pos(pos0), nq, nkv, h)
        assert got.dtype == dtype and tuple(got.shape) == (Bc, Tn, nq * h)
        assert torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(caches[1]), _bits(caches[0]))
        assert not (_bits(caches[1])[:, :, pos0:pos0 + Tn] == pattern).all() and (_bits(caches[1])[:, :, pos0 + Tn:] == pattern).all()
    finally:
        nn.set_compute_dtype(torch.float32)


# ---- one capture, many positions ------------------------------------------------------------------------------------------------------------------------
def test_one_captured_graph_follows_the_position(cuda, bf16):
    """rope + attention captured ONCE with *pos_d = 5; 70 and then 299 written into pos_d and replayed: each replay is the eager call at that
    position, in the output and in the cache.  A capture that froze the position would give the answer of position 5 three times."""
    from iseg_amd import functional as F

    Bc, Sc, nq, nkv, h = 1, 300, 8, 1, 256
    x = rnd((Bc, 1, (nq + 2 * nkv) * h), 7).to(torch.bfloat16).cuda()
    filled = rnd((Bc, 2, Sc, nkv, h), 8).to(torch.bfloat16).cuda()
    cache = filled.clone()
    pos_d = _pos(5)

    def step():
        return F.gemma_cached_attention_core(F.gemma_rope_cache(x, cache, pos_d, nq, nkv, h), cache, pos_d, nq, nkv, h)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()      # warm-up on the capture stream: the workspace may not grow under capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = step()
    seen = []
    for pos0 in (5, 70, 299):
        cache.copy_(filled)
        pos_d.fill_(pos0)
        graph.replay()
        ref_cache = filled.clone()
        want = F.gemma_cached_attention_core(F.gemma_rope_cache(x, ref_cache, pos0, nq, nkv, h), ref_cache, pos0, nq, nkv, h)
        assert torch.equal(_bits(out), _bits(want)), pos0
        assert torch.equal(_bits(cache), _bits(ref_cache)), pos0
        seen.append(out.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


# ---- guard bands, then out-of-range positions ---------------------------------------------------------------------------------------------------------------
def test_at_launchers_inside_guard_bands_and_out_of_range_positions(cuda, bf16):
    """as test_decode_attention_inside_guard_bands: operands (the position among them), the outputs and a workspace of EXACTLY the capacity's
    scratch bytes between bands of poison.  In-range positions leave the bands intact and give the unguarded result.  Only then, in the same
    arena, positions -1, S - Tn + 1 and S: the bands, the outputs, the workspace and the cache keep their bytes."""
    from iseg_amd import kernels as K

    for case in ((2, 130, 63, 2, 8, 1, 256, 0), (1, 192, 127, 2, 8, 1, 256, 3), (2, 65, 64, 1, 4, 2, 128, 0)):
        Bc, Sc, pos0, Tn, nq, nkv, h, splits = case
        scale = float(h) ** -0.5
        q = rnd((Bc, Tn, nq * h), 1).to(torch.bfloat16)
        x = rnd((Bc, Tn, (nq + 2 * nkv) * h), 3).to(torch.bfloat16)
        cache = rnd((Bc, 2, Sc, nkv, h), 2).to(torch.bfloat16)
        cache[:, :, pos0 + Tn:] = float("nan")
        table = torch.rand(Sc, h)
        plain_cache = cache.cuda()
        plain_q = K.gemma_rope_cache(x.cuda(), plain_cache, table.cuda(), pos0, nq, nkv, h)
        plain = K.gemma_decode_attention(q.cuda(), plain_cache, pos0, nq, nkv, h, scale, splits)
        arena = GM.Arena(cuda, 16 << 20)
        with GM.guarded(arena):
            qd, xd = arena.alloc(q.shape, q.dtype, "operand"), arena.alloc(x.shape, x.dtype, "operand")
            cd, td = arena.alloc(cache.shape, cache.dtype, "operand"), arena.alloc(table.shape, table.dtype, "operand")
            pd = arena.alloc((1,), torch.int32, "operand")
            for d, s_ in ((qd, q), (xd, x), (cd, cache), (td, table)):
                d.copy_(s_)
            pd.fill_(pos0)
            rq = K.gemma_rope_cache_at(xd, cd, td, pd, nq, nkv, h)
            y = K.gemma_decode_attention_at(qd, cd, pd, nq, nkv, h, scale, splits)
            arena.check()
            ws = [r for r in arena.records if r.role == "workspace"]
            assert len(ws) == 1
            assert ws[0].end - ws[0].start == K._hip.lib().iseg_gemma_decode_attention_scratch_bytes(Bc, Sc - Tn, Tn, nq, nkv, h, splits)
            assert torch.equal(_bits(rq.cpu()), _bits(plain_q.cpu())) and torch.equal(_bits(y.cpu()), _bits(plain.cpu()))
            assert torch.equal(_bits(cd.cpu()), _bits(plain_cache.cpu()))
            # the in-range position has passed: now the positions the host cannot refuse
            before = _bits(cd).clone()
            for bad in (-1, Sc - Tn + 1, Sc):
                mark = len(arena.records)
                pd.fill_(bad)
                K.gemma_rope_cache_at(xd, cd, td, pd, nq, nkv, h)
                K.gemma_decode_attention_at(qd, cd, pd, nq, nkv, h, scale, splits)
                arena.check()
                assert arena.untouched("output", since=mark) == (2, 2), bad
                assert arena.untouched("workspace") == (1, 1), bad
                assert torch.equal(_bits(cd), before) and int(pd.item()) == bad


def test_at_entry_points_refuse_what_the_host_can_check(cuda):
    """a null position and Tn > S are ISEG_ERR_ARG, fp32 and h = 96 ISEG_ERR_UNSUPPORTED, a workspace one byte short ISEG_ERR_WORKSPACE; the
    output, the workspace and the cache keep their poison"""
    from iseg_amd import _hip
    from iseg_amd import kernels as K

    L = _hip.lib()
    Bc, Sc, nq, nkv, h = 2, 130, 8, 1, 256
    out = torch.empty(Bc * 2 * nq * h, dtype=torch.bfloat16, device="cuda")
    cache = torch.empty(Bc, 2, Sc, nkv, h, dtype=torch.bfloat16, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    _bits(out).fill_(0x7FA5)
    _bits(cache).fill_(0x7FA5)
    ws.fill_(0xA5)
    q = torch.zeros(Bc * 2 * nq * h, dtype=torch.bfloat16, device="cuda")
    pos_d = _pos(0)
    need = L.iseg_gemma_decode_attention_scratch_bytes(Bc, Sc - 1, 1, nq, nkv, h, 0)

    def status(pos_ptr, Tn=1, S_=Sc, h_=h, code=_hip.BF16, nbytes=ws.numel()):
        return L.iseg_gemma_decode_attention_at(q.data_ptr(), nq * h_, cache[:, 0].data_ptr(), cache.stride(0), cache.stride(2), cache[:, 1].data_ptr(),
                                                cache.stride(0), cache.stride(2), out.data_ptr(), nq * h_, ws.data_ptr(), nbytes, Bc, S_, pos_ptr, Tn, nq,
                                                nkv, h_, float(h_) ** -0.5, 0, code, K.stream())

    assert status(None) == -1 and status(pos_d.data_ptr(), Tn=2, S_=1) == -1
    assert status(pos_d.data_ptr(), code=_hip.F32) == -3 and status(pos_d.data_ptr(), h_=96) == -3
    assert status(pos_d.data_ptr(), nbytes=need - 1) == -4 and "workspace" in _hip.last_error()
    table = torch.zeros(Sc, h, device="cuda")
    rc = L.iseg_gemma_rope_cache_at(q.data_ptr(), (nq + 2 * nkv) * h, out.data_ptr(), nq * h, cache[:, 0].data_ptr(), cache.stride(0), cache.stride(2),
                                    cache[:, 1].data_ptr(), cache.stride(0), cache.stride(2), table.data_ptr(), Bc, Sc, None, 1, nq, nkv, h, _hip.BF16,
                                    K.stream())
    assert rc == -1
    torch.cuda.synchronize()
    assert bool((_bits(out) == 0x7FA5).all()) and bool((_bits(cache) == 0x7FA5).all()) and bool((ws == 0xA5).all())


# ---- the commit kernel against the Python state machine ------------------------------------------------------------------------------------------------------
END = 7


def _commit_state(Bc, ids_dtype, end, seed):
    g = torch.Generator().manual_seed(seed)
    Sc = 8
    lengths = torch.randint(1, 5, (Bc,), generator=g)
    lengths[0] = 2      # index = 2 at the latest
    if Bc > 1:
        lengths[-1] = 4      # a row that holds user tokens at positions the loop visits
    mask = torch.arange(Sc)[None, :] < lengths[:, None]
    prompt = torch.where(mask, torch.randint(8, 90, (Bc, Sc), generator=g), torch.zeros((), dtype=torch.int64)).to(ids_dtype)
    index = int(lengths.min())
    st = R.State(prompt.tolist(), mask.tolist(), index, end)
    dev = dict(prompt=prompt.cuda(), mask=mask.cuda(), pos=_pos(index - 1), cur_ids=prompt[:, index - 1].contiguous().cuda(),
               done=torch.tensor(st.done).cuda())
    return st, dev, g


def _same(st, dev):
    return (dev["prompt"].tolist() == st.prompt and int(dev["pos"].item()) == st.pos and dev["cur_ids"].tolist() == st.cur_ids
            and dev["done"].tolist() == st.done)


@pytest.mark.parametrize("ids_dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("Bc", [1, 3, 300])
def test_decode_commit_follows_the_python_state_machine(cuda, Bc, ids_dtype):
    """S = 8, ragged user prefixes of 1 .. 4 tokens.  First run, with an end token: random tokens (user tokens must be kept), the end token
    handed to rows 1, 4, 7, .. at index 4 (done turns on for those rows alone) and to every row at index 5 (all done); every later launch is
    frozen.  Second run, without an end token: runs to p + 1 == S and freezes there.  After EVERY launch the device state is the restatement's.
    Tokens come as int64 (torch.argmax's type) in one run and as int32 (F.sample_tokens') in the other."""
    from iseg_amd import functional as F

    st, dev, g = _commit_state(Bc, ids_dtype, END, 11 + Bc)
    assert _same(st, dev)
    kept = 0
    for launch in range(9):
        tokens = torch.randint(8, 90, (Bc,), generator=g)
        col = st.pos + 1
        if col == 4:
            tokens[1::3] = END
        if col == 5:
            tokens[:] = END
        kept += sum(1 for b in range(Bc) if not R.frozen(st) and st.mask[b][col])
        moved = R.commit(st, tokens.tolist())
        F.decode_commit(dev["prompt"], dev["mask"], dev["pos"], dev["cur_ids"], dev["done"], tokens.cuda(), END)
        assert _same(st, dev), launch
        assert moved == (col <= 5)
    assert st.pos == 5 and all(st.done) and R.frozen(st) and (kept >= 1 or Bc == 1)
    # an out-of-range position is frozen as well
    for bad in (-2, 7, 8, 1 << 20):
        dev["pos"].fill_(bad)
        dev["done"].zero_()
        snapshot = (dev["prompt"].clone(), dev["cur_ids"].clone())
        F.decode_commit(dev["prompt"], dev["mask"], dev["pos"], dev["cur_ids"], dev["done"], torch.full((Bc,), 5).cuda(), END)
        assert int(dev["pos"].item()) == bad and torch.equal(dev["prompt"], snapshot[0]) and torch.equal(dev["cur_ids"], snapshot[1])
        assert not bool(dev["done"].any())

    st, dev, g = _commit_state(Bc, ids_dtype, None, 23 + Bc)
    for launch in range(10):
        tokens = torch.randint(0, 90, (Bc,), generator=g).to(torch.int32)      # the end token of the other run is just a token here
        col = st.pos + 1
        moved = R.commit(st, tokens.tolist())
        F.decode_commit(dev["prompt"], dev["mask"], dev["pos"], dev["cur_ids"], dev["done"], tokens.cuda())
        assert _same(st, dev), launch
        assert moved == (col < 8)
    assert st.pos == 7 and not any(st.done)


# ---- generation: the acceptance test --------------------------------------------------------------------------------------------------------------------------
def _sampler(kind):
    from iseg_amd.nlp import samplers as S_

    return {"greedy": lambda: "greedy", "top_k": lambda: S_.TopKSampler(k=5, seed=7), "top_p": lambda: S_.TopPSampler(p=0.9, seed=7),
            "random": lambda: S_.RandomSampler(seed=7)}[kind]()


def _generate(model, kind, graph, inputs, end=None, **kw):
    model.compile(sampler=_sampler(kind), graph_decode=graph)      # a fresh sampler: the same seed, the stream from its start
    out = model.generate_step(inputs, end_token_id=end, **kw)
    return out["token_ids"].cpu(), out["padding_mask"].cpu()


def _graphs(model):
    return sum(len(e["graphs"]) for e in model._decode_graphs.values())


@pytest.mark.parametrize("with_end", [False, True], ids=["no_end_token", "end_token"])
@pytest.mark.parametrize("kind", ["greedy", "top_k", "top_p", "random"])
def test_graphed_generation_is_the_eager_generation(cuda, bf16, kind, with_end):
    """the 2-layer model and the ragged prompts (5 and 9 tokens of 40) of tests/test_gemma_cache_gpu.py: graph_decode=True gives the token ids
    and the padding mask of graph_decode=False, torch.equal, for check_every 1 and 16; with_end: the end token is one the eager run emits before
    the end (row 0's third generated token, as test_greedy_generation picks it).  Other prompts of the same shape reuse the graph; after
    release_decode_graphs() it is captured again."""
    model, _ = _model(torch.bfloat16)
    ids, mask = _prompts()
    ids = ids * mask
    inputs = {"token_ids": ids.cuda(), "padding_mask": mask.cuda()}
    end = None
    if with_end:
        end = int(_generate(model, kind, False, inputs)[0][0, PROMPTS[0] + 2].item())
    want, want_mask = _generate(model, kind, False, inputs, end)
    if with_end:
        assert bool(((want == end) & ~mask).any()) and not want_mask.all()
    assert model._decode_graphs == {}
    for check_every in (1, 16):
        got, got_mask = _generate(model, kind, True, inputs, end, check_every=check_every)
        assert torch.equal(got, want) and torch.equal(got_mask, want_mask), check_every
        assert len(model._decode_graphs) == 1 and _graphs(model) == 1
    assert torch.equal(inputs["token_ids"].cpu(), ids)      # the caller's tensors are not written

    # other prompts of the same shape and type (the same signature): 5 and 7 tokens
    other = torch.randint(1, 97, (B, S), generator=torch.Generator().manual_seed(5))
    other_mask = torch.zeros(B, S, dtype=torch.bool)
    other_mask[:, :PROMPTS[0]] = True
    other_mask[1, :PROMPTS[0] + 2] = True
    other = other * other_mask
    inputs2 = {"token_ids": other.cuda(), "padding_mask": other_mask.cuda()}
    want2, want2_mask = _generate(model, kind, False, inputs2, end)
    got2, got2_mask = _generate(model, kind, True, inputs2, end)
    assert torch.equal(got2, want2) and torch.equal(got2_mask, want2_mask)
    assert not torch.equal(want2, want) and _graphs(model) == 1      # reused

    model.release_decode_graphs()
    assert model._decode_graphs == {}
    got3, got3_mask = _generate(model, kind, True, inputs, end)
    assert torch.equal(got3, want) and torch.equal(got3_mask, want_mask) and _graphs(model) == 1


def test_every_row_done_freezes_the_replays(cuda, bf16):
    """two identical rows, greedy: both emit the end token at the same step, the eager loop stops there, and the graphed loop, which looks only
    every 16 replays, must give the same tokens: the replays after the stop are frozen"""
    model, _ = _model(torch.bfloat16)
    ids, mask = _prompts()
    ids, mask = ids[:1].repeat(B, 1), mask[:1].repeat(B, 1)
    ids = ids * mask
    inputs = {"token_ids": ids.cuda(), "padding_mask": mask.cuda()}
    free, _ = _generate(model, "greedy", False, inputs)
    end = int(free[0, PROMPTS[0] + 2].item())
    want, want_mask = _generate(model, "greedy", False, inputs, end)
    stop = int(((want == end) & ~mask).float().argmax(dim=-1).max().item())
    assert bool(((want == end) & ~mask).any(dim=-1).all()) and stop < S - 2
    assert torch.equal(want[:, stop + 1:], ids[:, stop + 1:])      # the eager loop stopped: the padding is still there
    for check_every in (1, 3, 16):
        got, got_mask = _generate(model, "greedy", True, inputs, end, check_every=check_every)
        assert torch.equal(got, want) and torch.equal(got_mask, want_mask), check_every


def test_the_replay_loop_reads_nothing_back_without_an_end_token(cuda, bf16, monkeypatch):
    """a capture fails on any host synchronisation, so the captured step is proven free of host reads by existing (the idiom of
    test_update_state_replays_from_a_captured_graph_without_a_host_read); what is left is the loop around graph.replay(): every way a tensor
    reaches the host, and every synchronisation, raises while it runs.  With an end token the same loop reads `done` every check_every replays."""
    from iseg_amd.nlp import samplers as S_

    model, _ = _model(torch.bfloat16)
    ids, mask = _prompts()
    inputs = {"token_ids": (ids * mask).cuda(), "padding_mask": mask.cuda()}
    inner = model._replay_decode
    reads = []

    def guarded_loop(graph, e, steps, with_end, draw, check_every):
        def refuse(*a, **k):
            reads.append(1)
            if not with_end:
                raise AssertionError("the replay loop read the device on the host")
            return True

        with monkeypatch.context() as m:
            for name in ("item", "tolist", "cpu", "numpy", "__bool__"):
                m.setattr(torch.Tensor, name, refuse)
            m.setattr(torch.cuda, "synchronize", refuse)
            m.setattr(torch.cuda.Stream, "synchronize", refuse)
            m.setattr(torch.cuda.Event, "synchronize", refuse)
            return inner(graph, e, steps, with_end, draw, check_every)

    model._replay_decode = guarded_loop
    model.compile(sampler=S_.TopKSampler(k=5, seed=7), graph_decode=True)
    out = model.generate_step(inputs)["token_ids"].cpu()
    assert reads == [] and _graphs(model) == 1
    model.compile(sampler=S_.TopKSampler(k=5, seed=7), graph_decode=False)
    assert torch.equal(out, model.generate_step(inputs)["token_ids"].cpu())
    # with an end token: `refuse` answers "every row is done" at the first look, after check_every replays
    model.compile(sampler=S_.TopKSampler(k=5, seed=7), graph_decode=True)
    model.generate_step(inputs, end_token_id=96, check_every=4)
    assert len(reads) == 1


def test_graph_decode_refuses_the_fp32_compute_dtype(cuda):
    from iseg_amd import nn

    nn.set_compute_dtype(torch.float32)
    nn.set_device("cuda:0")
    model, _ = _model(torch.float32)
    ids, mask = _prompts()
    inputs = {"token_ids": (ids * mask).cuda(), "padding_mask": mask.cuda()}
    model.compile(graph_decode=True)
    with pytest.raises(ValueError, match="compute dtype is torch.float32"):
        model.generate_step(inputs)
    model.compile()
    assert tuple(model.generate_step(inputs)["token_ids"].shape) == (B, S)      # the default still runs the composed route
