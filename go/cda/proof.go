//go:build rocm

package cda

/*
#include "cda.h"
*/
import "C"

import (
	"fmt"
	"unsafe"
)

// Nodes is every node of the trees the block path builds for one square (cda_extend_commit_nodes): what
// pkg/inclusion's EDSSubTreeRootCacher records through nmt's NodeVisitor (pkg/inclusion/nmt_caching.go:76-124) and
// what pkg/proof recomputes for proofs (pkg/proof/proof.go:82-153).
type Nodes struct {
	K        int
	RowRoots [][]byte
	ColRoots [][]byte
	DataHash []byte
	// RowNodes[t] / ColNodes[t]: tree t's 4k-1 nodes of 90 bytes, the 2k leaves first, then each level, the root last
	RowNodes [][][]byte
	ColNodes [][][]byte
	// DAHNodes: the RFC-6962 tree over rowRoots ‖ colRoots (8k-1 nodes of 32 bytes), leaf hashes first, the data
	// root last
	DAHNodes [][]byte
}

// Node returns node `pos` of level `level` (0 = leaves) of a tree's flattened node list (w leaves).
func Node(tree [][]byte, w, level, pos int) []byte {
	off := 0
	for l := 0; l < level; l++ {
		off += w >> l
	}
	return tree[off+pos]
}

// ExtendCommitNodes extends the k*k shares and returns every row tree node (and, with cols / dahTree, the column
// trees' and the DAH tree's) from one GPU call.
func ExtendCommitNodes(ctx *Context, s [][]byte, cols, dahTree bool) (*Nodes, error) {
	if !isPowerOfTwo(len(s)) {
		return nil, fmt.Errorf("number of shares is not a power of 2: got %d", len(s))
	}
	flat, n, err := flatten(s)
	if err != nil {
		return nil, err
	}
	k := squareSize(len(s))
	w := 2 * k
	per := (2*w - 1) * NodeSize
	rows := make([]byte, w*NodeSize)
	colr := make([]byte, w*NodeSize)
	dah := make([]byte, 32)
	rn := make([]byte, w*per)
	var cn, dn []byte
	if cols {
		cn = make([]byte, w*per)
	}
	if dahTree {
		dn = make([]byte, (4*w-1)*32)
	}
	var info C.cda_err_info
	rc := C.cda_extend_commit_nodes(ctx.c, C.uint32_t(len(s)), C.uint32_t(n), ptr(flat), nil, ptr(rows), ptr(colr),
		ptr(dah), ptr(rn), ptr(cn), ptr(dn), &info)
	if rc != 0 {
		return nil, toErr(rc, &info)
	}
	out := &Nodes{K: k, RowRoots: split(rows, w), ColRoots: split(colr, w), DataHash: dah}
	out.RowNodes = make([][][]byte, w)
	for t := range out.RowNodes {
		out.RowNodes[t] = split(rn[t*per:(t+1)*per], 2*w-1)
	}
	if cols {
		out.ColNodes = make([][][]byte, w)
		for t := range out.ColNodes {
			out.ColNodes[t] = split(cn[t*per:(t+1)*per], 2*w-1)
		}
	}
	if dahTree {
		out.DAHNodes = split(dn, 4*w-1)
	}
	return out, nil
}

// RowProofPart is one proven row of a share inclusion proof: the row root, its RFC-6962 proof in the data root
// (merkle.ProofsFromByteSlices over rowRoots ‖ colRoots, proof.go:82-93) and the NMT range proof of the row's part
// of the range (tree.ProveRange, proof.go:129-152).
type RowProofPart struct {
	Row      int
	RowRoot  []byte
	Total    int64
	LeafHash []byte
	Aunts    [][]byte // bottom-up
	Start    int32
	End      int32
	Nodes    [][]byte // left to right
}

// ShareProofParts is pkg/proof NewShareInclusionProof's content for ODS shares [start, end): one GPU call extends the
// square, exports the nodes and assembles every proof (cda_share_inclusion_proof); no host hashing.
type ShareProofParts struct {
	StartRow, EndRow int
	Rows             []RowProofPart
	DataRoot         []byte
}

// ShareInclusionProof returns the proof parts of shares [start, end) of the square `s` (k*k shares).
func ShareInclusionProof(ctx *Context, s [][]byte, start, end int) (*ShareProofParts, error) {
	if !isPowerOfTwo(len(s)) {
		return nil, fmt.Errorf("number of shares is not a power of 2: got %d", len(s))
	}
	flat, n, err := flatten(s)
	if err != nil {
		return nil, err
	}
	k := squareSize(len(s))
	lg := 0
	for 1<<lg < 2*k {
		lg++
	}
	var info C.cda_share_proof_info
	rr := make([]byte, k*NodeSize)
	lh := make([]byte, k*32)
	au := make([]byte, k*(lg+1)*32)
	ns := make([]int32, 3*k)
	nodes := make([]byte, k*2*lg*NodeSize+1)
	root := make([]byte, 32)
	var e C.cda_err_info
	rc := C.cda_share_inclusion_proof(ctx.c, C.uint32_t(len(s)), C.uint32_t(n), ptr(flat), C.uint32_t(start),
		C.uint32_t(end), &info, ptr(rr), ptr(lh), ptr(au), (*C.int32_t)(unsafe.Pointer(&ns[0])),
		(*C.int32_t)(unsafe.Pointer(&ns[k])), (*C.int32_t)(unsafe.Pointer(&ns[2*k])), ptr(nodes), ptr(root), &e)
	if rc != 0 {
		return nil, toErr(rc, &e)
	}
	out := &ShareProofParts{StartRow: int(info.start_row), EndRow: int(info.end_row), DataRoot: root}
	maxNodes := int(info.max_nodes)
	for i := 0; i < int(info.nrows); i++ {
		p := RowProofPart{
			Row:      int(info.start_row) + i,
			RowRoot:  rr[i*NodeSize : (i+1)*NodeSize : (i+1)*NodeSize],
			Total:    int64(info.total),
			LeafHash: lh[i*32 : (i+1)*32 : (i+1)*32],
			Start:    ns[i],
			End:      ns[k+i],
		}
		for a := 0; a < int(info.naunts); a++ {
			o := (i*(lg+1) + a) * 32
			p.Aunts = append(p.Aunts, au[o:o+32:o+32])
		}
		for j := 0; j < int(ns[2*k+i]); j++ {
			o := (i*maxNodes + j) * NodeSize
			p.Nodes = append(p.Nodes, nodes[o:o+NodeSize:o+NodeSize])
		}
		out.Rows = append(out.Rows, p)
	}
	return out, nil
}

// RetainedSquare is one extended block kept on the device (cda_square_open): the EDS, every node of its 4k trees and
// the RFC-6962 tree over rowRoots ‖ colRoots.  It answers any number of share-range proofs per call without
// extending or hashing again.  Close it when the block is no longer served; closing after the context was closed is
// safe.
type RetainedSquare struct {
	h        *C.cda_square
	K        int
	RowRoots [][]byte
	ColRoots [][]byte
	DataHash []byte
}

// OpenSquare extends and commits the k*k shares once (da.ExtendShares + NewDataAvailabilityHeader) and keeps the
// square on the device.
func OpenSquare(ctx *Context, s [][]byte) (*RetainedSquare, error) {
	if !isPowerOfTwo(len(s)) {
		return nil, fmt.Errorf("number of shares is not a power of 2: got %d", len(s))
	}
	flat, n, err := flatten(s)
	if err != nil {
		return nil, err
	}
	k := squareSize(len(s))
	w := 2 * k
	rows := make([]byte, w*NodeSize)
	cols := make([]byte, w*NodeSize)
	dah := make([]byte, 32)
	var h *C.cda_square
	var info C.cda_err_info
	rc := C.cda_square_open(ctx.c, C.uint32_t(len(s)), C.uint32_t(n), ptr(flat), &h, ptr(rows), ptr(cols), ptr(dah),
		&info)
	if rc != 0 {
		return nil, toErr(rc, &info)
	}
	return &RetainedSquare{h: h, K: k, RowRoots: split(rows, w), ColRoots: split(cols, w), DataHash: dah}, nil
}

// Close releases the square's device memory.
func (sq *RetainedSquare) Close() {
	if sq.h != nil {
		C.cda_square_close(sq.h)
		sq.h = nil
	}
}

// ShareRange is shares.Range over the ODS, row-major: [Start, End).
type ShareRange struct {
	Start, End int
}

// SquareShareProof is one proof of a ShareProofs batch: the proved shares (ShareProof.Data) and the parts of its rows.
type SquareShareProof struct {
	Data [][]byte
	ShareProofParts
}

// ShareProofs is pkg/proof NewShareInclusionProof (proof.go:55-167) for every range from ONE launch
// (cda_square_share_proofs): each proof's NMT range proofs, row roots and the row roots' proofs in the data root are
// gathered from the retained nodes.
func (sq *RetainedSquare) ShareProofs(ranges []ShareRange) ([]SquareShareProof, error) {
	if sq.h == nil {
		return nil, fmt.Errorf("cda: square is closed")
	}
	if len(ranges) == 0 {
		return nil, nil
	}
	k := sq.K
	lg := 0
	for 1<<lg < 2*k {
		lg++
	}
	maxNodes, naunts := 2*lg, lg+1
	if maxNodes == 0 {
		maxNodes = 1
	}
	q := make([]C.cda_share_range, len(ranges))
	nrows, nshares := 0, 0
	for i, r := range ranges {
		if r.Start < 0 || r.Start >= r.End || r.End > k*k {
			return nil, fmt.Errorf("cda: share range [%d, %d) outside the %d x %d square", r.Start, r.End, k, k)
		}
		q[i].start, q[i].end = C.uint32_t(r.Start), C.uint32_t(r.End)
		nrows += (r.End-1)/k - r.Start/k + 1
		nshares += r.End - r.Start
	}
	rowOff := make([]uint32, len(ranges)+1)
	recs := make([]C.cda_share_row, nrows)
	nodes := make([]byte, nrows*maxNodes*NodeSize)
	rr := make([]byte, nrows*NodeSize)
	lh := make([]byte, nrows*32)
	au := make([]byte, nrows*naunts*32)
	shares := make([]byte, nshares*ShareSize)
	root := make([]byte, 32)
	rc := C.cda_square_share_proofs(sq.h, C.uint32_t(len(q)), &q[0], C.uint32_t(maxNodes), C.uint32_t(nrows),
		(*C.uint32_t)(unsafe.Pointer(&rowOff[0])), &recs[0], ptr(nodes), ptr(rr), ptr(lh), ptr(au), ptr(shares),
		C.uint64_t(len(shares)), ptr(root))
	if rc != 0 {
		return nil, toErr(rc, nil)
	}
	out := make([]SquareShareProof, len(ranges))
	cursor := 0
	for i, r := range ranges {
		p := &out[i]
		p.DataRoot = root
		p.Data = split(shares[cursor*ShareSize:(cursor+r.End-r.Start)*ShareSize], r.End-r.Start)
		cursor += r.End - r.Start
		lo, hi := int(rowOff[i]), int(rowOff[i+1])
		p.StartRow, p.EndRow = int(recs[lo].row), int(recs[hi-1].row)
		for j := lo; j < hi; j++ {
			rec := &recs[j]
			part := RowProofPart{
				Row:      int(rec.row),
				RowRoot:  rr[j*NodeSize : (j+1)*NodeSize : (j+1)*NodeSize],
				Total:    int64(rec.total),
				LeafHash: lh[j*32 : (j+1)*32 : (j+1)*32],
				Start:    int32(rec.nmt_start),
				End:      int32(rec.nmt_end),
			}
			for a := 0; a < int(rec.naunts); a++ {
				o := (int(rec.aunt_off) + a) * 32
				part.Aunts = append(part.Aunts, au[o:o+32:o+32])
			}
			for t := 0; t < int(rec.nnodes); t++ {
				o := (int(rec.node_off) + t) * NodeSize
				part.Nodes = append(part.Nodes, nodes[o:o+NodeSize:o+NodeSize])
			}
			p.Rows = append(p.Rows, part)
		}
	}
	return out, nil
}

// ShareProofVerdict is the first check of ShareProof.Validate (share_proof.go:16-51) that a proof fails, 0 if none
// (the CDA_SP_* codes of cda.h).
type ShareProofVerdict int32

// ValidateShareProofs is ShareProof.Validate of a batch on the GPU (cda_share_proofs_validate): proof i under the
// 29-byte namespace namespaces[i] against dataRoots[i].  A false proof is a verdict, never an error.
func ValidateShareProofs(ctx *Context, proofs []SquareShareProof, namespaces [][]byte,
	dataRoots [][]byte) ([]ShareProofVerdict, error) {
	if len(proofs) == 0 {
		return nil, nil
	}
	if len(namespaces) != len(proofs) || len(dataRoots) != len(proofs) {
		return nil, fmt.Errorf("cda: %d proofs, %d namespaces, %d data roots", len(proofs), len(namespaces),
			len(dataRoots))
	}
	descs := make([]C.cda_share_proof_desc, len(proofs))
	var recs []C.cda_share_row
	var rr, lh, nodes, aunts, leaves, roots []byte
	nnodes, naunts, nleaves := 0, 0, 0
	for i := range proofs {
		p := &proofs[i]
		if len(namespaces[i]) != NamespaceSize || len(dataRoots[i]) != 32 {
			return nil, fmt.Errorf("cda: proof %d: namespace of %d bytes, data root of %d", i, len(namespaces[i]),
				len(dataRoots[i]))
		}
		d := &descs[i]
		d.row_off = C.uint32_t(len(recs))
		d.nshare_proofs, d.nrow_roots, d.nrow_proofs = C.uint32_t(len(p.Rows)), C.uint32_t(len(p.Rows)),
			C.uint32_t(len(p.Rows))
		d.leaf_off, d.nleaves = C.uint32_t(nleaves), C.uint32_t(len(p.Data))
		d.start_row, d.end_row = C.uint32_t(p.StartRow), C.uint32_t(p.EndRow)
		d.data_root = C.uint32_t(i)
		for j := 0; j < NamespaceSize; j++ {
			d.ns[j] = C.uint8_t(namespaces[i][j])
		}
		roots = append(roots, dataRoots[i]...)
		for _, s := range p.Data {
			if len(s) != ShareSize {
				return nil, fmt.Errorf("cda: proof %d: share of %d bytes", i, len(s))
			}
			leaves = append(leaves, s...)
		}
		nleaves += len(p.Data)
		for _, row := range p.Rows {
			if len(row.RowRoot) != NodeSize || len(row.LeafHash) != 32 {
				return nil, fmt.Errorf("cda: proof %d: row root of %d bytes, leaf hash of %d", i, len(row.RowRoot),
					len(row.LeafHash))
			}
			var rec C.cda_share_row
			rec.nmt_start, rec.nmt_end = C.int32_t(row.Start), C.int32_t(row.End)
			rec.node_off, rec.nnodes = C.uint32_t(nnodes), C.uint32_t(len(row.Nodes))
			rec.total, rec.index = C.int64_t(row.Total), C.int64_t(row.Row)
			rec.aunt_off, rec.naunts = C.uint32_t(naunts), C.uint32_t(len(row.Aunts))
			rec.row = C.uint32_t(row.Row)
			recs = append(recs, rec)
			rr = append(rr, row.RowRoot...)
			lh = append(lh, row.LeafHash...)
			for _, x := range row.Nodes {
				if len(x) != NodeSize {
					return nil, fmt.Errorf("cda: proof %d: node of %d bytes", i, len(x))
				}
				nodes = append(nodes, x...)
			}
			for _, x := range row.Aunts {
				if len(x) != 32 {
					return nil, fmt.Errorf("cda: proof %d: aunt of %d bytes", i, len(x))
				}
				aunts = append(aunts, x...)
			}
			nnodes += len(row.Nodes)
			naunts += len(row.Aunts)
		}
	}
	verdicts := make([]ShareProofVerdict, len(proofs))
	var recp *C.cda_share_row
	if len(recs) > 0 {
		recp = &recs[0]
	}
	rc := C.cda_share_proofs_validate(ctx.c, C.uint32_t(len(descs)), &descs[0], recp, ptr(rr), ptr(lh),
		C.uint32_t(len(recs)), ptr(nodes), C.uint32_t(nnodes), ptr(aunts), C.uint32_t(naunts), ptr(leaves),
		C.uint32_t(nleaves), ptr(roots), C.uint32_t(len(proofs)), (*C.int32_t)(unsafe.Pointer(&verdicts[0])))
	if rc != 0 {
		return nil, toErr(rc, nil)
	}
	return verdicts, nil
}

// NamespaceProofKind says what ProveNamespace found in a tree (the CDA_NSP_* codes of cda.h).
type NamespaceProofKind uint32

const (
	// NamespaceEmpty: the namespace lies outside the tree root's [min, max]; the proof has no nodes.
	NamespaceEmpty NamespaceProofKind = 0
	// NamespaceInclusion: Shares are all the tree's leaves of the namespace, [Start, End) their range.
	NamespaceInclusion NamespaceProofKind = 1
	// NamespaceAbsence: inside the root's range but not present; LeafHash is the node of the first leaf with a
	// larger namespace, [Start, Start+1) its range.
	NamespaceAbsence NamespaceProofKind = 2
)

// NamespaceQuery asks tree (Axis, Index) of the extended square for everything of a 29-byte namespace.
type NamespaceQuery struct {
	Axis, Index int
	Namespace   []byte
}

// NamespaceProof is nmt's ProveNamespace result for one tree: the namespace's shares (inclusion only) and the proof
// that they are all of them (proof.pb.go NMTProof: Start, End, Nodes, LeafHash).
type NamespaceProof struct {
	Kind       NamespaceProofKind
	Start, End int
	Nodes      [][]byte // left to right
	LeafHash   []byte   // nil unless Kind == NamespaceAbsence
	Shares     [][]byte
}

// ProveNamespace is nmt's Tree.ProveNamespace for every query from ONE call (cda_square_prove_namespace): the
// namespace's run is found in the retained leaf records on the device, the nodes are gathered from the retained
// trees, the shares copied from the retained EDS.
func (sq *RetainedSquare) ProveNamespace(queries []NamespaceQuery) ([]NamespaceProof, error) {
	if sq.h == nil {
		return nil, fmt.Errorf("cda: square is closed")
	}
	if len(queries) == 0 {
		return nil, nil
	}
	w := 2 * sq.K
	lg := 0
	for 1<<lg < w {
		lg++
	}
	maxNodes := 2 * lg
	q := make([]C.cda_namespace_query, len(queries))
	for i, x := range queries {
		if x.Axis < 0 || x.Axis > 1 || x.Index < 0 || x.Index >= w || len(x.Namespace) != NamespaceSize {
			return nil, fmt.Errorf("cda: namespace query %d: axis %d, index %d, namespace of %d bytes", i, x.Axis,
				x.Index, len(x.Namespace))
		}
		q[i].axis, q[i].index = C.uint32_t(x.Axis), C.uint32_t(x.Index)
		for j := 0; j < NamespaceSize; j++ {
			q[i].ns[j] = C.uint8_t(x.Namespace[j])
		}
	}
	res := make([]C.cda_namespace_result, len(q))
	nodes := make([]byte, len(q)*maxNodes*NodeSize)
	lh := make([]byte, len(q)*NodeSize)
	// nq * 2k * 512 bytes always suffice; ask for the proofs first and size the share buffer from the total
	var total C.uint64_t
	rc := C.cda_square_prove_namespace(sq.h, C.uint32_t(len(q)), &q[0], C.uint32_t(maxNodes), &res[0], ptr(nodes),
		ptr(lh), nil, 0, &total)
	if rc != 0 {
		return nil, toErr(rc, nil)
	}
	var shares []byte
	if total > 0 {
		shares = make([]byte, int(total)*ShareSize)
		rc = C.cda_square_prove_namespace(sq.h, C.uint32_t(len(q)), &q[0], C.uint32_t(maxNodes), &res[0], ptr(nodes),
			ptr(lh), ptr(shares), C.uint64_t(len(shares)), &total)
		if rc != 0 {
			return nil, toErr(rc, nil)
		}
	}
	out := make([]NamespaceProof, len(q))
	for i := range out {
		r := &res[i]
		p := &out[i]
		p.Kind, p.Start, p.End = NamespaceProofKind(r.kind), int(r.start), int(r.end)
		for j := 0; j < int(r.nnodes); j++ {
			o := (i*maxNodes + j) * NodeSize
			p.Nodes = append(p.Nodes, nodes[o:o+NodeSize:o+NodeSize])
		}
		if p.Kind == NamespaceAbsence {
			p.LeafHash = lh[i*NodeSize : (i+1)*NodeSize : (i+1)*NodeSize]
		}
		if n := int(r.nshares); n > 0 {
			o := int(r.share_off) * ShareSize
			p.Shares = split(shares[o:o+n*ShareSize], n)
		}
	}
	return out, nil
}

// VerifyNamespace is nmt's Proof.VerifyNamespace of a batch on the GPU (cda_nmt_verify_namespace): proof i claims
// that proofs[i].Shares are ALL the leaves of namespaces[i] in the tree with root roots[i] (90 bytes).  Completeness
// is part of the verdict: an inclusion proof of a part of the namespace's run is false.  A false proof is a verdict,
// never an error.
func VerifyNamespace(ctx *Context, proofs []NamespaceProof, namespaces [][]byte, roots [][]byte) ([]bool, error) {
	if len(proofs) == 0 {
		return nil, nil
	}
	if len(namespaces) != len(proofs) || len(roots) != len(proofs) {
		return nil, fmt.Errorf("cda: %d proofs, %d namespaces, %d roots", len(proofs), len(namespaces), len(roots))
	}
	descs := make([]C.cda_nmt_ns_proof_desc, len(proofs))
	var ns, rr, nodes, lhs, leaves []byte
	nnodes, nlh, nleaves := 0, 0, 0
	for i := range proofs {
		p := &proofs[i]
		if len(namespaces[i]) != NamespaceSize || len(roots[i]) != NodeSize || p.Start < 0 || p.End < 0 {
			return nil, fmt.Errorf("cda: proof %d: namespace of %d bytes, root of %d, range [%d, %d)", i,
				len(namespaces[i]), len(roots[i]), p.Start, p.End)
		}
		d := &descs[i]
		d.start, d.end = C.uint32_t(p.Start), C.uint32_t(p.End)
		d.node_off, d.nnodes = C.uint32_t(nnodes), C.uint32_t(len(p.Nodes))
		d.leaf_off, d.nleaves = C.uint32_t(nleaves), C.uint32_t(len(p.Shares))
		d.root = C.uint32_t(i)
		d.leaf_hash = C.CDA_NO_LEAF_HASH
		if len(p.LeafHash) != 0 {
			if len(p.LeafHash) != NodeSize {
				return nil, fmt.Errorf("cda: proof %d: leaf hash of %d bytes", i, len(p.LeafHash))
			}
			d.leaf_hash = C.uint32_t(nlh)
			lhs = append(lhs, p.LeafHash...)
			nlh++
		}
		ns = append(ns, namespaces[i]...)
		rr = append(rr, roots[i]...)
		for _, x := range p.Nodes {
			if len(x) != NodeSize {
				return nil, fmt.Errorf("cda: proof %d: node of %d bytes", i, len(x))
			}
			nodes = append(nodes, x...)
		}
		for _, s := range p.Shares {
			if len(s) != ShareSize {
				return nil, fmt.Errorf("cda: proof %d: share of %d bytes", i, len(s))
			}
			leaves = append(leaves, s...)
		}
		nnodes += len(p.Nodes)
		nleaves += len(p.Shares)
	}
	ok := make([]byte, len(proofs))
	rc := C.cda_nmt_verify_namespace(ctx.c, C.uint32_t(len(descs)), &descs[0], ptr(ns), ptr(rr),
		C.uint32_t(len(proofs)), ptr(nodes), C.uint32_t(nnodes), ptr(lhs), C.uint32_t(nlh), ptr(leaves),
		C.uint32_t(nleaves), ptr(ok))
	if rc != 0 {
		return nil, toErr(rc, nil)
	}
	out := make([]bool, len(ok))
	for i, v := range ok {
		out[i] = v == 1
	}
	return out, nil
}
