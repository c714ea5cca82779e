"""Import name of FBGEMM's GPU package for the reference's `import fbgemm_gpu` (examples/commons/ops/length_to_offsets.py:15),
which is there for its side effect: the `torch.ops.fbgemm.*` ops exist afterwards.  This package only imports
`fbgemm_jagged_ops` next to it, which registers the ops that examples/hstu calls, over the gfx950 kernels of this library.
It is not FBGEMM and has no other content; where the real fbgemm_gpu is installed it comes first on sys.path or, imported
first, keeps its ops (fbgemm_jagged_ops leaves a registered op alone)."""
import fbgemm_jagged_ops  # noqa: F401
