"""The voxel integrator (nidreg_integrator_*, csrc/nid_voxel_kernels.hpp, csrc/nidreg_voxel.hip) at the edges its first tests
(tests/test_voxel_gpu.py) leave out: the chunk loop of one insert, probe chains that share home slots and cross the end of the
table, the width of the radix sort, coordinates exactly on a boundary, and the upload layouts of the C ABI.

Every comparison is EXACT, as in tests/test_voxel_gpu.py: uint32 views of the records, equal sequence numbers.  The large cases are
compared with preprocess_oracle.winners_numpy, which a CPU test below pins to the dict oracle bit for bit.  Each input that has
to satisfy a condition has a CPU test that checks the condition without a GPU.

The shapes are tied to constants of csrc/nidreg_voxel.hip that ``info()`` does not expose; whoever changes one reshapes the tests
that name it."""
import numpy as np
import pytest

import preprocess_oracle
from direct_visual_lidar_calibration_amd import _lib, preprocess
from test_voxel_gpu import MIN_D, RES, assert_equals_oracle, parity_oracle

K_CHUNK = 1 << 20       # kChunk of csrc/nidreg_voxel.hip: points per claim / payload launch pair of one insert
INITIAL_CAP = 1 << 16   # kInitialCap: slots of a fresh table (checked against info() where a test relies on it)
TAIL = 65               # points of the second chunk: one wave and one lane more


class Restated:
    """winners_numpy over a list of frames behind the interface assert_equals_oracle reads"""

    def __init__(self, frames, res, min_distance):
        self.rec, self.seq, self.vox, self.offered = preprocess_oracle.winners_numpy(frames, res, min_distance)

    def winners(self):
        return self.rec, self.seq, self.vox

    def size(self):
        return len(self.seq)


def records_of(points, intensities):
    """the stored 16-byte float32 record: both views of it take the upload-as-it-lies route"""
    rec = np.concatenate([points, intensities[:, None]], axis=1).astype(np.float32)
    return rec[:, :3], rec[:, 3]


# ---- A0 -------------------------------------------------------------------------------------------------------------------------


def ragged_frames():
    """the three-stage sequence of test_voxel_gpu.test_ragged_frames_growth_and_revisits, as frames"""
    res, min_d = 0.05, 0.5
    rng = np.random.default_rng(5)
    frames = []
    for n in (0, 1, 63, 64, 65, 4097):
        frames.append((rng.uniform(-1.5, 1.5, (n, 3)), rng.uniform(0, 1, n)))
    o = preprocess_oracle.Integrator(res, min_d)
    for f in frames:
        o.insert(*f)
    early_vox = o.winners()[2]
    i = np.arange(200000) % (60 * 60 * 42)
    vox = np.stack([i % 60 + 80, (i // 60) % 60 - 30, i // 3600 - 21], axis=1)
    frames.append(((vox + 0.5) * res, rng.uniform(0, 1, 200000)))
    pick = early_vox[np.linalg.norm((early_vox + 0.5) * res, axis=1) > min_d + 0.1][:1000]
    frames.append(((pick + 0.5) * res, 2.0 + rng.uniform(0, 1, 1000)))
    return frames, res, min_d


def test_the_numpy_oracle_equals_the_dict_oracle_bit_for_bit():
    """(CPU, A0) winners_numpy == Integrator.winners() -- records as uint32, sequence numbers, voxels, offered -- on the parity
    input (double and float32) and on the frames of test_ragged_frames_growth_and_revisits."""
    c = parity_oracle()
    cases = [([(c["points"], c["intensities"])], RES, MIN_D), ([(c["points"].astype(np.float32), c["intensities"].astype(np.float32))], RES, MIN_D), ragged_frames()]
    cases.append(([(np.zeros((0, 3)), np.zeros(0))], RES, MIN_D))
    cases.append(([(np.array([[-0.0, 0.0, 0.0], [0.0, -0.0, -0.0]]), np.array([1.0, 2.0]))], RES, 0.0))  # one voxel, as one dict key
    for frames, res, min_d in cases:
        o = preprocess_oracle.Integrator(res, min_d)
        for f in frames:
            o.insert(*f)
        rec_o, seq_o, vox_o = o.winners()
        rec, seq, vox, offered = preprocess_oracle.winners_numpy(frames, res, min_d)
        assert offered == o.offered and rec.dtype == np.float32 and seq.dtype == np.int64
        assert np.array_equal(seq, seq_o) and np.array_equal(vox, vox_o) and np.array_equal(rec.view(np.uint32), rec_o.view(np.uint32))
    assert len(seq) == 1 and seq[0] == 1


# ---- A1: the chunk loop with growth between the chunks ----------------------------------------------------------------------------

_cache = {}


def growth_input():
    """2^20 lattice voxels of 128 x 128 x 64 at resolution 0.05, 2 m and more in front (min_distance 1), one point at the centre of
    each in shuffled order; then 65 of those voxels again, at their centres, with intensities >= 2.  float32 records."""
    if "growth" not in _cache:
        rng = np.random.default_rng(41)
        i = rng.permutation(K_CHUNK)
        vox = np.stack([i % 128 + 40, (i // 128) % 128 - 64, i // 16384 - 32], axis=1)
        again = rng.choice(K_CHUNK, size=TAIL, replace=False)
        vox = np.concatenate([vox, vox[again]])
        inten = np.concatenate([rng.uniform(0, 1, K_CHUNK), 2.0 + np.arange(TAIL) / 128.0])
        points, intensities = records_of((vox + 0.5) * 0.05, inten)
        _cache["growth"] = dict(points=points, intensities=intensities, vox=vox, again=again, oracle=Restated([(points, intensities)], 0.05, 1.0))
    return _cache["growth"]


def test_the_growth_input_is_a_lattice_of_distinct_voxel_centres():
    """(CPU, A1) As float32 the 2^20 + 65 points still sit within 1e-5 of a voxel centre in units of the resolution, 1 m and more
    beyond the gate; the first 2^20 voxels are distinct and the oracle's winners are all of them, the last 65 the revisits."""
    c = growth_input()
    q = c["points"].astype(np.float64) / 0.05
    assert np.abs(q - np.floor(q) - 0.5).max() < 1e-5
    assert np.linalg.norm(c["points"].astype(np.float64), axis=1).min() > 2.0
    assert len(np.unique(c["vox"][:K_CHUNK], axis=0)) == K_CHUNK
    o = c["oracle"]
    assert o.size() == K_CHUNK and o.offered == K_CHUNK + TAIL
    assert np.array_equal(o.seq[-TAIL:], np.arange(K_CHUNK, K_CHUNK + TAIL)) and np.array_equal(o.vox[-TAIL:], c["vox"][-TAIL:])
    assert not np.isin(c["again"], o.seq).any()


def check_growth(points, intensities):
    c = growth_input()
    first = preprocess.StaticPointCloudIntegrator(0.05, 1.0, device=0)
    assert first.info()["capacity"] == INITIAL_CAP
    first.insert_points(points[:K_CHUNK], intensities[:K_CHUNK])
    cap_first = first.info()["capacity"]
    assert first.size() == K_CHUNK
    assert cap_first == 2 * K_CHUNK, "one chunk of 2^20 new voxels no longer ends at 2^21 slots: kChunk or the growth rule changed, reshape this test"
    first.close()
    integ = preprocess.StaticPointCloudIntegrator(0.05, 1.0, device=0)
    integ.insert_points(points, intensities)
    rec = assert_equals_oracle(integ, c["oracle"])
    info = integ.info()
    assert info["voxels"] == K_CHUNK and info["offered"] == K_CHUNK + TAIL
    assert info["capacity"] >= 2 * info["voxels"]
    assert info["capacity"] > cap_first  # the table was rehashed between the two chunks of ONE insert
    assert np.array_equal(integ.last_seq[-TAIL:], np.arange(K_CHUNK, K_CHUNK + TAIL))
    assert np.array_equal(rec[-TAIL:, 3], (2.0 + np.arange(TAIL) / 128.0).astype(np.float32)) and (rec[:-TAIL, 3] < 2.0).all()
    integ.close()


@pytest.mark.gpu
def test_second_chunk_of_one_insert_after_a_rehash_float_route():
    """(A1) One frame of kChunk + 65 points (kChunk = 2^20 of csrc/nidreg_voxel.hip; the shape is tied to it): the first chunk fills
    2^20 voxels, the size read back before the second chunk makes vox_reserve rehash a table that holds the first chunk's
    payloads, and the 65 points of the second chunk (i0 = 2^20, sequence numbers 2^20 .. 2^20 + 64, slot scratch reused) must
    find their voxels at the new slots and overwrite them."""
    c = growth_input()
    check_growth(c["points"], c["intensities"])


@pytest.mark.gpu
def test_second_chunk_of_one_insert_after_a_rehash_double_route():
    """(A1) The same values widened to double (kChunk as above).  Both routes are compared with the same oracle bytes, so the two
    give identical bytes."""
    c = growth_input()
    check_growth(c["points"].astype(np.float64), c["intensities"].astype(np.float64))


# ---- A2, A3: the chunk loop without growth, and a third chunk with sequence numbers carried over --------------------------------


def crowded_input():
    """Two frames of 2^20 + 65 float32 points at resolution 0.25, min_distance 1: the first falls into 1000 voxels of a 10^3 block
    2 m in front, the second into 1500 voxels of a 10 x 10 x 15 block that shares the first 1000; positions uniform inside the
    voxel, 0.01 of its edge away from its faces."""
    if "crowded" not in _cache:
        rng = np.random.default_rng(42)
        frames, ids = [], []
        for nvox in (1000, 1500):
            v = rng.integers(0, nvox, K_CHUNK + TAIL)
            vox = np.stack([v % 10 + 8, (v // 10) % 10 - 5, v // 100 - 5], axis=1)
            pts = (vox + rng.uniform(0.01, 0.99, (K_CHUNK + TAIL, 3))) * 0.25
            frames.append(records_of(pts, rng.uniform(0, 1, K_CHUNK + TAIL)))
            ids.append(v)
        _cache["crowded"] = dict(frames=frames, ids=ids, one=Restated(frames[:1], 0.25, 1.0), both=Restated(frames, 0.25, 1.0))
    return _cache["crowded"]


def last_occurrence(ids):
    order = np.arange(len(ids))
    last = np.full(ids.max() + 1, -1, dtype=np.int64)
    np.maximum.at(last, ids, order)
    return np.sort(last[last >= 0])


def test_the_crowded_input_keeps_the_margins_of_the_parity_input():
    """(CPU, A2 / A3) Every float32 point is further than 1.3e-3 from the distance gate and every quotient further than 3e-6 from
    an integer (the criteria of test_the_parity_input_is_unambiguous); all 1000 voxels are hit in the first chunk already, the
    oracle's winners are the voxels' last occurrences, and some of them lie in the second chunk of either frame."""
    c = crowded_input()
    for pts, _ in c["frames"]:
        p = pts.astype(np.float64)
        q = p / 0.25
        gate, frac = np.abs(np.linalg.norm(p, axis=1) - 1.0).min(), np.abs(q - np.rint(q)).min()
        print(f"closest to the gate {gate:.3e}, closest quotient to an integer {frac:.3e}")
        assert gate > 1.3e-3 and frac > 3e-6
    a, b = c["ids"]
    assert len(np.unique(a[:K_CHUNK])) == 1000 and c["one"].size() == 1000 and c["both"].size() == 1500
    assert np.array_equal(c["one"].seq, last_occurrence(a))
    assert ((c["one"].seq >= K_CHUNK).sum() > 0) and ((c["one"].seq < K_CHUNK).sum() > 0)
    n = K_CHUNK + TAIL
    assert np.array_equal(c["both"].seq, last_occurrence(np.concatenate([a, b])))  # (a voxel has the same number in both frames)
    assert (c["both"].seq >= n + K_CHUNK).sum() > 0 and c["both"].offered == 2 * n


@pytest.mark.gpu
def test_second_chunk_of_one_insert_without_growth():
    """(A2) kChunk + 65 points (kChunk = 2^20; the shape is tied to it) in 1000 voxels: the read-back before the second chunk
    LOWERS the bound from 2^20 to 1000 and the table stays as it is; winners come from both chunks."""
    c = crowded_input()
    pts, inten = c["frames"][0]
    first = preprocess.StaticPointCloudIntegrator(0.25, 1.0, device=0)
    first.insert_points(pts[:K_CHUNK], inten[:K_CHUNK])
    cap_first = first.info()["capacity"]
    assert first.size() == 1000
    # the table is grown ahead for a whole chunk of new voxels: 2 * kChunk slots for a frame of exactly one chunk.  Another value
    # means kChunk (or the growth rule) changed and the frame below no longer is "one chunk and 65 points": reshape this test
    assert cap_first == 2 * K_CHUNK, "the premise of this test (kChunk = 2^20) is gone"
    first.close()
    integ = preprocess.StaticPointCloudIntegrator(0.25, 1.0, device=0)
    integ.insert_points(pts, inten)
    assert_equals_oracle(integ, c["one"])
    assert integ.info()["capacity"] == cap_first and integ.info()["offered"] == K_CHUNK + TAIL
    seq = integ.last_seq
    assert np.array_equal(seq, last_occurrence(c["ids"][0]))
    assert ((seq >= K_CHUNK) & (seq < K_CHUNK + TAIL)).any() and (seq < K_CHUNK).any()
    integ.close()


@pytest.mark.gpu
def test_third_chunk_carries_the_sequence_numbers_over_from_the_first_frame():
    """(A3) A second frame of kChunk + 65 points (kChunk = 2^20; the shape is tied to it) into the integrator of A2: its second
    chunk runs with seq0 = offered + i0, both terms non-zero."""
    c = crowded_input()
    integ = preprocess.StaticPointCloudIntegrator(0.25, 1.0, device=0)
    for pts, inten in c["frames"]:
        integ.insert_points(pts, inten)
        if integ.info()["offered"] == K_CHUNK + TAIL:  # (as in A2: a table grown ahead for exactly one chunk)
            assert integ.info()["capacity"] == 2 * K_CHUNK, "the premise of this test (kChunk = 2^20) is gone"
    assert_equals_oracle(integ, c["both"])
    n = K_CHUNK + TAIL
    assert integ.info()["offered"] == 2 * n and (integ.last_seq >= n + K_CHUNK).any()
    integ.close()


# ---- A4: shared home slots and a probe chain across the end of the table (white box) ---------------------------------------------


def cluster_input():
    """Voxels of [-64, 64)^3 by their home slot in a table of kInitialCap = 2^16 slots: all whose home is one of the LAST 8 slots,
    and 1000 of those whose home is one of the FIRST 256.  Three points per voxel, shuffled, resolution 0.25, min_distance 0."""
    if "cluster" not in _cache:
        g = np.arange(-64, 64)
        vox = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
        home = preprocess_oracle.home_slot(vox, INITIAL_CAP)
        tail, head = vox[home >= INITIAL_CAP - 8], vox[home < 256]
        rng = np.random.default_rng(43)
        chosen = np.concatenate([tail, head[rng.choice(len(head), size=1000, replace=False)]])
        v = np.repeat(chosen, 3, axis=0)[rng.permutation(3 * len(chosen))]
        pts = (v + rng.uniform(0.1, 0.9, v.shape)) * 0.25
        inten = rng.uniform(0, 1, len(pts))
        # the frame that makes the table grow: 40 000 voxel centres further out, none of them among the chosen
        i = np.arange(40000)
        far = np.stack([i % 40 + 100, (i // 40) % 40 - 20, i // 1600 - 12], axis=1)
        grow = ((far + 0.5) * 0.25, rng.uniform(0, 1, 40000))
        _cache["cluster"] = dict(tail=tail, head=head, home=home, chosen=chosen, vox=v, frames=[(pts, inten), grow])
    return _cache["cluster"]


def test_the_cluster_input_shares_home_slots_and_wraps_around_the_table():
    """(CPU, A4) The restated hash gives the counts of candidates computed when the test was written -- 288 voxels home in the last 8
    slots, 36 of them in slot 65535, 8226 in the first 256 --, and linear probing over the chosen keys, in the order of the frame
    and in the reverse of it, ends on both sides of the wrap: keys that start in the last 8 slots end in the first slots, and keys
    that live in the first slots are pushed off their home by them."""
    c = cluster_input()
    assert len(c["tail"]) >= 200 and len(c["head"]) >= 1000
    assert (len(c["tail"]), int((c["home"] == INITIAL_CAP - 1).sum()), len(c["head"])) == (288, 36, 8226)
    assert len(np.unique(preprocess_oracle.packed_key(c["chosen"]))) == len(c["chosen"]) == 1288
    _, first = np.unique(preprocess_oracle.packed_key(c["vox"]), return_index=True)
    for order in (np.sort(first), np.sort(first)[::-1]):
        keys_vox = c["vox"][order]
        home = preprocess_oracle.home_slot(keys_vox, INITIAL_CAP)
        slot = preprocess_oracle.linear_probe(home, INITIAL_CAP)
        from_tail = home >= INITIAL_CAP - 8
        assert (slot[from_tail] >= INITIAL_CAP - 8).sum() == 8       # the last 8 slots are all taken ...
        assert (slot[from_tail] < 2048).sum() == 280                 # ... and 280 keys went round the end of the table,
        assert (slot[~from_tail] != home[~from_tail]).sum() > 280    # into one cluster with the keys that live there
        assert slot.max() == INITIAL_CAP - 1 and slot[slot < INITIAL_CAP - 8].max() < 2048
    # whole waves compete: every window of 64 consecutive points of the frame (a wave is one of them) holds several DISTINCT keys
    # whose home is one of the last 8 slots
    home_of_point = preprocess_oracle.home_slot(c["vox"], INITIAL_CAP)
    key_of_point = preprocess_oracle.packed_key(c["vox"])
    fewest = min(len(np.unique(key_of_point[s : s + 64][home_of_point[s : s + 64] >= INITIAL_CAP - 8])) for s in range(len(key_of_point) - 63))
    print(f"fewest distinct keys homed in the last 8 slots in any 64-point window: {fewest}")
    assert fewest >= 2


@pytest.mark.gpu
def test_probe_chains_that_share_home_slots_and_cross_the_end_of_the_table():
    """(A4, white box: kInitialCap = 2^16 slots, vox_mix and the packed key as restated in preprocess_oracle) 288 keys whose home
    is one of the last 8 slots and 1000 whose home is one of the first 256, three points each in one frame: the chain runs through
    slot 65535 into slot 0 and interleaves with the keys that live there, and the lanes of a wave lose the compare-and-swap on
    the same empty slots to each other's keys.  Then a frame that grows the table rehashes the cluster."""
    c = cluster_input()
    integ = preprocess.StaticPointCloudIntegrator(0.25, 0.0, device=0)
    assert integ.info()["capacity"] == INITIAL_CAP, "the table no longer starts at 2^16 slots: the home slots of this test are not the table's"
    integ.insert_points(*c["frames"][0])
    assert integ.info()["capacity"] == INITIAL_CAP, "the table grew during the frame: the cluster was not built in 2^16 slots"
    assert_equals_oracle(integ, Restated(c["frames"][:1], 0.25, 0.0))
    assert integ.size() == 1288
    integ.insert_points(*c["frames"][1])
    assert integ.info()["capacity"] > INITIAL_CAP
    assert_equals_oracle(integ, Restated(c["frames"], 0.25, 0.0))
    assert integ.size() == 1288 + 40000
    integ.close()


# ---- A5: the width of the radix sort -----------------------------------------------------------------------------------------------


def sort_width_frames():
    """Frames whose totals are 2^16, 2^16 + 1, 2^17 and 2^17 + 1 offered points; all points crowd into 500 voxels except the LAST
    of each total, which has a voxel of its own (resolution 0.25, min_distance 0)."""
    rng = np.random.default_rng(44)
    frames, own = [], 0
    for n in (40000, (1 << 16) - 40000, 1, 30001, (1 << 16) - 30002, 1):
        v = rng.integers(0, 500, n)
        vox = np.stack([v % 10, (v // 10) % 10, v // 100], axis=1).astype(np.float64)
        own += 1
        vox[-1] = (40 + own, -3, 7)
        frames.append(((vox + rng.uniform(0.1, 0.9, (n, 3))) * 0.25, rng.uniform(0, 1, n)))
    return frames


def test_the_sort_width_totals_are_powers_of_two_with_a_last_voxel_of_its_own():
    """(CPU, A5)"""
    frames = sort_width_frames()
    totals = np.cumsum([len(w) for _, w in frames]).tolist()
    assert [totals[i] for i in (1, 2, 4, 5)] == [1 << 16, (1 << 16) + 1, 1 << 17, (1 << 17) + 1]
    for upto in (2, 3, 5, 6):
        o = Restated(frames[:upto], 0.25, 0.0)
        assert o.seq[-1] == o.offered - 1 and (np.diff(o.seq) > 0).all()
        assert not (o.vox[:-1] == o.vox[-1]).all(axis=1).any()


@pytest.mark.gpu
def test_sort_width_when_the_largest_key_is_a_power_of_two():
    """(A5) nidreg_integrator_get sorts keys = sequence number + 1 with end_bit derived from `offered`; at offered = 2^16 and 2^17
    with the last point the winner of a voxel of its own, the largest key IS `offered` and needs one more bit than `offered - 1`.
    One total of 2^k + 1 each as well.  (No constant of the kernels shapes this test: the totals are powers of two themselves.)"""
    frames = sort_width_frames()
    integ = preprocess.StaticPointCloudIntegrator(0.25, 0.0, device=0)
    for upto, frame in enumerate(frames, start=1):
        integ.insert_points(*frame)
        if upto in (2, 3, 5, 6):
            o = Restated(frames[:upto], 0.25, 0.0)
            assert_equals_oracle(integ, o)
            assert integ.info()["offered"] == o.offered
            assert (np.diff(integ.last_seq) > 0).all() and integ.last_seq[-1] == o.offered - 1
    integ.close()


# ---- A6: exact boundaries -----------------------------------------------------------------------------------------------------------

B_RES, B_MIN = 0.25, 5.0
B_K = [-2.0, -1.0, -0.0, 0.0, 1.0]


def boundary_points():
    """Per axis a: the five coordinates k * 0.25 on that axis, 8.0 (voxel 32) on the next one, 0 on the third"""
    pts = []
    for a in range(3):
        for k in B_K:
            p = [0.0, 0.0, 0.0]
            p[a], p[(a + 1) % 3] = k * B_RES, 8.0
            pts.append(p)
    return np.array(pts)


ON_THE_GATE = np.array([[3.0, 4.0, 0.0], [0.0, -3.0, 4.0], [-4.0, 0.0, 3.0]])


def test_the_boundary_input_is_exact_in_either_summation_order():
    """(CPU, A6) k * 0.25 / 0.25 == k exactly; the three points on the gate have norm exactly 5.0 whether the squares are summed
    x^2 + (y^2 + z^2) (the kernel, Eigen) or (x^2 + y^2) + z^2 (the oracle); (3, 4, 0) (1 - 2^-52) has a norm below 5.0 in both."""
    p = boundary_points()
    assert np.array_equal(p / B_RES, p * 4.0) and np.signbit(p[2, 0]) and not np.signbit(p[3, 0])
    inside = ON_THE_GATE[0] * (1.0 - 2.0**-52)
    for q, want in ((ON_THE_GATE, [5.0, 5.0, 5.0]), (inside[None], None)):
        x, y, z = q[:, 0], q[:, 1], q[:, 2]
        for norm in (np.sqrt(x * x + (y * y + z * z)), np.sqrt((x * x + y * y) + z * z)):
            if want is not None:
                assert norm.tolist() == want
            else:
                assert norm[0] < 5.0
    o = preprocess_oracle.Integrator(B_RES, B_MIN)
    o.insert(p, np.arange(15.0))
    assert o.size() == 12  # -0.0 and +0.0 are one voxel on every axis
    vox = o.winners()[2]
    for a in range(3):
        assert sorted(vox[vox[:, (a + 1) % 3] == 32][:, a].tolist()) == [-2, -1, 0, 1]


@pytest.mark.gpu
def test_coordinates_exactly_on_a_voxel_face_and_norms_exactly_on_the_gate():
    """(A6) Coordinates that are exact multiples of the resolution, -0.0 and -res among them, land in voxel k (floor, -0.0 merges with
    +0.0 and the later point wins); a norm that EQUALS min_distance is kept (the gate is a strict <), the next double below is
    dropped.  Double and float32 routes (every value is a float32)."""
    p = np.concatenate([boundary_points(), ON_THE_GATE, ON_THE_GATE[:1] * (1.0 - 2.0**-52)])
    w = np.arange(len(p), dtype=np.float64)
    o = preprocess_oracle.Integrator(B_RES, B_MIN)
    assert o.insert(p, w) == 18 and o.size() == 15
    integ = preprocess.StaticPointCloudIntegrator(B_RES, B_MIN, device=0)
    integ.insert_points(p, w)
    rec = assert_equals_oracle(integ, o)
    assert set(rec[:, 3].tolist()) == set(range(19)) - {2.0, 7.0, 12.0, 18.0}  # the -0.0 points lost to +0.0; the last is gated
    integ.close()
    # float32: the point just inside the gate is not a float32, the rest is exact
    integ = preprocess.StaticPointCloudIntegrator(B_RES, B_MIN, device=0)
    integ.insert_points(p[:18].astype(np.float32), w[:18].astype(np.float32))
    assert np.array_equal(integ.get_records().view(np.uint32), rec.view(np.uint32)) and np.array_equal(integ.last_seq, o.winners()[1])
    integ.close()
    # the same five on one axis with the gate at 0: the origin (norm 0, not < 0) is kept
    line = np.zeros((5, 3))
    line[:, 0] = np.array(B_K) * B_RES
    o0 = preprocess_oracle.Integrator(B_RES, 0.0)
    o0.insert(line, np.arange(5.0))
    integ = preprocess.StaticPointCloudIntegrator(B_RES, 0.0, device=0)
    integ.insert_points(line, np.arange(5.0))
    rec0 = assert_equals_oracle(integ, o0)
    assert rec0[:, 3].tolist() == [0.0, 1.0, 3.0, 4.0] and np.array_equal(o0.winners()[2][:, 0], [-2, -1, 0, 1])
    integ.close()


@pytest.mark.gpu
def test_overflowing_squares_and_infinities_are_refused_and_nothing_is_inserted():
    """(A6) 1e200 squared overflows: the norm is infinite, the point passes the gate and its voxel is out of range; 3e38 as float32
    does not overflow as a double square and is merely out of range; +-inf is counted as non-finite."""
    c = parity_oracle()
    integ = preprocess.StaticPointCloudIntegrator(RES, MIN_D, device=0)
    integ.insert_points(c["points"][:500], c["intensities"][:500])
    rec, seq = integ.get_records(), integ.last_seq
    cases = []
    for value, dtype, message in ((1e200, np.float64, "0 point(s) with a non-finite coordinate, 1 point(s) outside the packed-key limit"),
                                  (-1e200, np.float64, "0 point(s) with a non-finite coordinate, 1 point(s) outside the packed-key limit"),
                                  (3e38, np.float32, "0 point(s) with a non-finite coordinate, 1 point(s) outside the packed-key limit"),
                                  (np.inf, np.float64, "1 point(s) with a non-finite coordinate, 0 point(s) outside the packed-key limit"),
                                  (-np.inf, np.float64, "1 point(s) with a non-finite coordinate, 0 point(s) outside the packed-key limit"),
                                  (np.inf, np.float32, "1 point(s) with a non-finite coordinate, 0 point(s) outside the packed-key limit")):
        bad = c["points"][500:600].astype(dtype)
        bad[41, 1] = value
        cases.append((bad, message))
    for bad, message in cases:
        with pytest.raises(ValueError) as e:
            integ.insert_points(bad, np.zeros(100, dtype=bad.dtype))
        assert message in str(e.value) and "nothing was inserted" in str(e.value), str(e.value)
        assert integ.info()["offered"] == 500 and np.array_equal(integ.get_records().view(np.uint32), rec.view(np.uint32)) and np.array_equal(integ.last_seq, seq)
    integ.close()


# ---- A7: layouts ------------------------------------------------------------------------------------------------------------------


@pytest.mark.gpu
def test_upload_layouts_of_the_c_abi_give_the_bytes_of_the_plain_route():
    """(A7) On the parity input: double points with stride 40 (the two-dimensional copy of 32 of every 40 bytes), float32 (n, 4)
    rows with separate intensities (packed on the host, point stride 16), float32 rows that are every other row of a larger array
    (point stride 24, intensity stride 8), nidreg_integrator_get without sequence numbers, and an integrator that only ever saw
    empty frames."""
    lib = _lib.load()
    c = parity_oracle()
    n = len(c["points"])
    plain = preprocess.StaticPointCloudIntegrator(RES, MIN_D, device=0)
    plain.insert_points(c["points"], c["intensities"])
    rec = assert_equals_oracle(plain, c["oracle"])
    seq = plain.last_seq

    # nidreg_integrator_get(seq = NULL): the same records
    only = np.full((len(rec), 4), np.nan, dtype=np.float32)
    assert lib.nidreg_integrator_get(plain._h, only.ctypes.data_as(_lib.c_float_p), None) == _lib.NIDREG_OK
    assert np.array_equal(only.view(np.uint32), rec.view(np.uint32))
    plain.close()

    wide = np.full((n, 5), 1e300)  # columns 3 and 4 must not be read as coordinates
    wide[:, :3] = c["points"]
    inten = np.ascontiguousarray(c["intensities"])
    g = preprocess.StaticPointCloudIntegrator(RES, MIN_D, device=0)
    assert wide.strides == (40, 8)
    assert lib.nidreg_integrator_insert(g._h, wide.ctypes.data, 40, inten.ctypes.data, n) == _lib.NIDREG_OK, _lib.last_error()
    assert np.array_equal(g.get_records().view(np.uint32), rec.view(np.uint32)) and np.array_equal(g.last_seq, seq)
    g.close()

    # float32: the plain route is the contiguous (n, 3) array with contiguous intensities
    p32, w32 = c["points"].astype(np.float32), c["intensities"].astype(np.float32)
    o32 = preprocess_oracle.Integrator(RES, MIN_D)
    o32.insert(p32, w32)
    g = preprocess.StaticPointCloudIntegrator(RES, MIN_D, device=0)
    g.insert_points(p32, w32)
    rec32, seq32 = assert_equals_oracle(g, o32), g.last_seq
    g.close()
    rows4 = np.concatenate([p32, np.full((n, 1), np.float32(1.0))], axis=1)
    big = np.full((2 * n, 3), np.float32(7e37))
    big[::2] = p32
    big_w = np.full(2 * n, np.float32(-1.0))
    big_w[::2] = w32
    assert rows4.strides == (16, 4) and big[::2].strides == (24, 4) and big_w[::2].strides == (8,)
    for points, intensities in ((rows4, w32), (big[::2], w32), (big[::2], big_w[::2])):
        g = preprocess.StaticPointCloudIntegrator(RES, MIN_D, device=0)
        g.insert_points(points, intensities)
        assert np.array_equal(g.get_records().view(np.uint32), rec32.view(np.uint32)) and np.array_equal(g.last_seq, seq32)
        g.close()

    # only empty frames, double and float32
    g = preprocess.StaticPointCloudIntegrator(RES, MIN_D, device=0)
    g.insert_points(np.zeros((0, 3)), np.zeros(0))
    g.insert_points(np.zeros((0, 4), dtype=np.float32), np.zeros(0, dtype=np.float32))
    assert g.size() == 0 and g.get_records().shape == (0, 4) and g.last_seq.shape == (0,) and g.info()["offered"] == 0
    assert lib.nidreg_integrator_get(g._h, None, None) == _lib.NIDREG_OK
    pts, inten = g.get_points()
    assert pts.shape == (0, 3) and inten.shape == (0,)
    g.close()
