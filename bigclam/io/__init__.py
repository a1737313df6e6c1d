from .cover import Cover, load_cover, read_cover_lines
from .edgelist import Graph, build_graph, load_graph, parse_edge_array
from .synthetic import (
    planted_overlap,
    planted_partition,
    rmat_edges,
    rmat_graph,
    rmat_graph_with_edges,
    shaped_graph,
)

__all__ = [
    "Cover",
    "Graph",
    "build_graph",
    "load_graph",
    "load_cover",
    "parse_edge_array",
    "planted_overlap",
    "planted_partition",
    "read_cover_lines",
    "rmat_edges",
    "rmat_graph",
    "rmat_graph_with_edges",
    "shaped_graph",
]
