"""TEST / BENCH HARNESS (not the engine): the copy-constraint side of the reference's PlonkStructure, restated in Python so
that the device permutation check (mira_amd/decider.py) can be fed matrices built the reference's way.

* `Assembly` -- src/plonk/permutation.rs:18-95 (adapted there from halo2's keygen): every cell starts in a cycle of its own;
  `copy` merges the cycles of two cells, the smaller into the larger;
* `cell_to_z_idx`, `construct_permutation_matrix`, `fill_sparse_matrix` -- src/plonk/util.rs:13-71, 128-174: the triples of
  the N x N matrix P, N = num_io + num_rows * num_advice, with P Z = Z iff the copy constraints hold for
  Z = instance || advice columns;
* `matrix_multiply` -- src/polynomial/sparse.rs:7-19, on Python integers.

Columns are plain (kind, index) tuples, kind "instance" or "advice" (a fixed column is not allowed in a copy constraint:
the reference panics).  The reference holds no literal vector for any of these functions, so this restatement is what
"the reference's value" means for the permutation check."""

INSTANCE, ADVICE, FIXED = "instance", "advice", "fixed"


class Assembly:
    """columns: the columns that take part in the permutation argument (cs.permutation.columns); n: rows per column"""

    def __init__(self, n, columns):
        self.columns = list(columns)
        cols = [[(i, j) for j in range(n)] for i in range(len(self.columns))]
        self.mapping = [list(c) for c in cols]
        self.aux = [list(c) for c in cols]
        self.sizes = [[1] * n for _ in self.columns]

    def copy(self, left_column, left_row, right_column, right_row):
        if left_column not in self.columns or right_column not in self.columns:
            raise KeyError("ColumnNotInPermutation")
        lc, rc = self.columns.index(left_column), self.columns.index(right_column)
        if left_row >= len(self.mapping[lc]) or right_row >= len(self.mapping[rc]):
            raise IndexError("BoundsFailure")
        left_cycle, right_cycle = self.aux[lc][left_row], self.aux[rc][right_row]
        if left_cycle == right_cycle:
            return
        if self.sizes[left_cycle[0]][left_cycle[1]] < self.sizes[right_cycle[0]][right_cycle[1]]:
            left_cycle, right_cycle = right_cycle, left_cycle
        self.sizes[left_cycle[0]][left_cycle[1]] += self.sizes[right_cycle[0]][right_cycle[1]]
        i = right_cycle
        while True:
            self.aux[i[0]][i[1]] = left_cycle
            i = self.mapping[i[0]][i[1]]
            if i == right_cycle:
                break
        self.mapping[lc][left_row], self.mapping[rc][right_row] = self.mapping[rc][right_row], self.mapping[lc][left_row]


def cell_to_z_idx(column, row, num_rows, num_io):
    if num_io > 0 and column >= 1:
        return num_io + (column - 1) * num_rows + row
    return row + column * num_rows


def _instance_column_index(columns):
    return next((i for i, c in enumerate(columns) if c[0] == INSTANCE), None)


def _column_index(column, has_instance):
    kind, index = column
    if kind == FIXED:
        raise ValueError("fixed column is not allowed in the copy constraint, it will break during folding")
    return index + (1 if kind == ADVICE and has_instance else 0)


def fill_sparse_matrix(triples, num_advice, num_rows, num_io, columns):
    """identity rows for every column that takes no part in the permutation argument"""
    num_columns = num_advice + 1 if num_io > 0 else num_advice
    has_instance = _instance_column_index(columns) is not None
    taken = {_column_index(c, has_instance) for c in columns}
    for col in sorted(set(range(num_columns)) - taken):          # (a HashSet in the reference: the order of the triples is not defined there)
        for row in range(num_rows):
            z = cell_to_z_idx(col, row, num_rows, num_io)
            triples.append((z, z, 1))
    return triples


def construct_permutation_matrix(k_table_size, num_io, num_advice, assembly):
    """-> [(row, col, 1)]: the SparseMatrix of PlonkStructure::permutation_matrix"""
    columns = assembly.columns
    inst = _instance_column_index(columns)
    num_rows = 1 << k_table_size
    triples = []
    for left_col, mapping_vec in enumerate(assembly.mapping):
        for left_row, cycle in enumerate(mapping_vec):
            if left_row >= num_io and left_col == inst:
                continue
            lc = _column_index(columns[left_col], inst is not None)
            rc = _column_index(columns[cycle[0]], inst is not None)
            triples.append((cell_to_z_idx(lc, left_row, num_rows, num_io), cell_to_z_idx(rc, cycle[1], num_rows, num_io), 1))
    return fill_sparse_matrix(triples, num_advice, num_rows, num_io, columns)


def matrix_multiply(triples, Z, mod):
    result = [0] * len(Z)
    for t in triples:
        row, col, value = t[0], t[1], (t[2] if len(t) > 2 and t[2] is not None else 1)
        if col >= len(Z):
            raise IndexError("invalid matrix multiply")
        result[row] = (result[row] + value * Z[col]) % mod
    return result


def perm_mismatches(triples, Z, mod):
    """is_sat_perm's count (src/plonk/mod.rs:577-583) and the lowest index that differs (None if none)"""
    y = matrix_multiply(triples, Z, mod)
    bad = [i for i, (a, b) in enumerate(zip(y, Z)) if (a - b) % mod]
    return len(bad), (bad[0] if bad else None)
