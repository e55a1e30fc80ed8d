"""Inputs of tests/test_gpu_wide_rings.py: tiny 6-D clouds whose same-stride kernel map has a chosen number of 64-pair
tiles, so that on a 64-compute-unit share (a grid of 64 persistent workgroups, eight per XCD) the busiest workgroup of
the wide conv kernel (conv_wide.hip) walks exactly `walk` tiles -- 1, 2, 3 and D - 1, D, D + 1 for the kernel's ring
depths in tiles: the gather sets and the index / scale registers (4 one-phase tiles, 2 two-phase tiles), the scale
distance (3, 4, 6), the index distance (5, 7, 11) and the 32 slots of the index / scale rings in LDS.

Two builders.  `dumbbells`: isolated pairs of voxels one kernel offset apart -- m dumbbells of offset k put exactly m pairs
into rule k and m into its mirror rule, and every voxel one pair into the centre rule, so rule sizes and the tile count
are chosen exactly.  `lattice_rows`: the first n voxels of a dense 4 x 3^5 box, whose rules hold up to 900 pairs -- thousands
of tiles from a few hundred rows.  Every case states its edge; the test asserts it from the library's own arrays."""
import numpy as np

from oracle import me_semantics as me

K = 729
SEED = 41   # of the synthetic 6-D checkpoint whose layers the cases run through
SHAPES = [(64, 64, 4, 'block2.conv1', 'block2.norm1'), (64, 128, 6, 'conv3', 'norm3'),
          (128, 128, 7, 'block3.conv1', 'block3.norm1'), (256, 128, 12, 'conv4_tr', 'norm4_tr'),
          (128, 256, 9, 'conv4', 'norm4'), (256, 256, 10, 'block4.conv1', 'block4.norm1')]   # cin, cout, layer, conv, norm


def share_walk(tiles):
    """tiles of the busiest workgroup of a 64-workgroup grid: an XCD gets ceil(T / 8) tiles, its eight workgroups deal them"""
    return -(-(-(-tiles // 8)) // 8)


def dumbbells(spec):
    """spec: [(number of offsets, dumbbells per offset)]; offsets taken from the first half of the 729 in order"""
    offs = me.kernel_offsets(6, 3)
    rows, g, k = [], 0, 0
    for count, m in spec:
        for _ in range(count):
            assert k < K // 2
            for _ in range(m):
                base = 4 * np.array([g % 64, (g // 64) % 64, g // 4096, 0, 0, 0]) + 1
                rows += [base, base + offs[k]]
                g += 1
            k += 1
    rows = np.asarray(rows, np.int32)
    return np.concatenate([np.zeros((len(rows), 1), np.int32), rows], axis=1)


def dumbbell_tiles(spec):
    return sum(2 * c * -(-m // 64) for c, m in spec) + -(-2 * sum(c * m for c, m in spec) // 64)


def lattice_rows(n):
    g = np.stack(np.meshgrid(*[np.arange(s) for s in (4, 3, 3, 3, 3, 3)], indexing='ij'), -1).reshape(-1, 6)[:n]
    return np.concatenate([np.zeros((len(g), 1), np.int32), g.astype(np.int32)], axis=1)


class Case:
    def __init__(self, name, make, walk=None, tiles=None, rule_sizes=()):
        self.name, self.make, self.walk, self.tiles, self.rule_sizes = name, make, walk, tiles, tuple(rule_sizes)
        self._coords = None

    @property
    def coords(self):
        if self._coords is None:
            self._coords = np.ascontiguousarray(self.make(), np.int32)
            assert len(np.unique(self._coords, axis=0)) == len(self._coords)
        return self._coords

    def features(self, cin):
        """rows of very different magnitude (four decades), both signs; the same in every process"""
        rng = np.random.default_rng([len(self.coords), cin])
        x = rng.standard_normal((len(self.coords), cin)) * 10.0 ** rng.uniform(-2, 2, (len(self.coords), 1))
        return x.astype(np.float32)

    def __repr__(self):
        return self.name


def _walk_case(n):
    spec = [(min(32 * n - (4 if n < 8 else 8), K // 2), 1)]
    assert share_walk(dumbbell_tiles(spec)) == n
    return Case(f'walk{n}', lambda: dumbbells(spec), walk=n, tiles=dumbbell_tiles(spec), rule_sizes=(1,))


CASES = [
    # XCD edges: fewer tiles than XCDs (three XCD ranges empty), and one more than eight (the fifth range holds one tile)
    Case('tiles5', lambda: dumbbells([(2, 1)]), walk=1, tiles=5, rule_sizes=(1,)),
    Case('tiles9', lambda: dumbbells([(4, 1)]), walk=1, tiles=9, rule_sizes=(1,)),
    # rules of 1, 63, 64 and 65 pairs (tiles: one short, one nearly full, one full, one full + one of a single pair)
    Case('rules_1_63_64_65', lambda: dumbbells([(1, 1), (1, 63), (1, 64), (1, 65)]), walk=1, tiles=17, rule_sizes=(1, 63, 64, 65)),
] + [_walk_case(n) for n in (1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12)] + [
    # the 32-slot rings wrap: dense rows, rules of up to 900 pairs
    Case('walk31', lambda: lattice_rows(672), walk=31),
    Case('walk32', lambda: lattice_rows(684), walk=32),
    Case('walk33', lambda: lattice_rows(686), walk=33),
]
