// KeywordPirClient on the device (reference Sources/PrivateInformationRetrieval/KeywordPir/KeywordPirProtocol.swift:279-392):
// generateQuery(at:using:) from resident keywords (he_keyword_client_generate_query_device), decrypt(response:at:using:) from
// resident replies to values (he_keyword_client_decrypt_response_device) and countEntriesInResponse
// (he_keyword_client_count_entries_device).  A thin wrapper: every buffer is the caller's DeviceBuffer, nothing is copied.
import CHeAmd
import HomomorphicEncryption

/// What `he_keyword_client_plan` says about one keyword database.
public struct GpuKeywordPirClientPlan: Sendable {
    public let expandedQueryCount: Int
    public let queryCiphertextCount: Int
    public let replyCiphertextCount: Int
    public let entriesPerPlaintext: Int
    public let bytesPerPlaintext: Int
    /// The longest value a bucket row holds: the stride of `values` in `decrypt`.
    public let valueCapacity: Int
    /// The bytes `countEntries` scans per reply.
    public let replyBytes: Int
}

/// `KeywordPirClient`: the `IndexPirParameter` of the keyword database as its fields and `hashFunctionCount`.
public struct GpuKeywordPirClient: @unchecked Sendable {
    /// `HashBucket.find`'s outcome per keyword, as `status` holds it.
    public enum Status: UInt32, Sendable {
        case notFound = 0
        case found = 1
        case corruptedData = 2
    }

    public let context: OpaquePointer
    public let wordBits: UInt32
    public let dimensions: [UInt32]
    /// `indexPirParameter.entryCount`: the cuckoo table's `bucketsPerTable`.
    public let entryCount: Int
    public let entrySizeInBytes: Int
    public let hashFunctionCount: UInt32
    public let plan: GpuKeywordPirClientPlan

    public init(context: OpaquePointer, wordBits: UInt32 = 64, dimensions: [UInt32], entryCount: Int, entrySizeInBytes: Int,
                hashFunctionCount: Int) throws
    {
        self.context = context
        self.wordBits = wordBits
        self.dimensions = dimensions
        self.entryCount = entryCount
        self.entrySizeInBytes = entrySizeInBytes
        self.hashFunctionCount = UInt32(hashFunctionCount)
        var expanded = 0, queryCiphertexts = 0, replyCiphertexts = 0, perPlaintext = 0, bytesPerPlaintext = 0
        var capacity = 0, replyBytes = 0
        try heAmdCheck(he_keyword_client_plan(context, dimensions, UInt32(dimensions.count), entryCount, entrySizeInBytes,
                                              UInt32(hashFunctionCount), &expanded, &queryCiphertexts, &replyCiphertexts,
                                              &perPlaintext, &bytesPerPlaintext, &capacity, nil, nil, &replyBytes))
        plan = GpuKeywordPirClientPlan(expandedQueryCount: expanded, queryCiphertextCount: queryCiphertexts,
                                       replyCiphertextCount: replyCiphertexts, entriesPerPlaintext: perPlaintext,
                                       bytesPerPlaintext: bytesPerPlaintext, valueCapacity: capacity, replyBytes: replyBytes)
    }

    private func bytes(_ buffer: DeviceBuffer) -> UnsafeMutablePointer<UInt8> {
        UnsafeMutableRawPointer(buffer.pointer).assumingMemoryBound(to: UInt8.self)
    }

    private func words(_ buffer: DeviceBuffer) -> UnsafeMutablePointer<UInt64> {
        UnsafeMutableRawPointer(buffer.pointer).assumingMemoryBound(to: UInt64.self)
    }

    /// `generateQuery(at:using:)` for `queries` keywords: `keywords` the blob, `keywordOffsets` uint64 [queries + 1], seeds
    /// [queries][C][32]; `out` [queries][C][2][L][N], `hashes` (optional) uint64 [queries] for the reply.
    public func generateQuery(keywords: DeviceBuffer, keywordOffsets: DeviceBuffer, queries: Int, secretKey: DeviceBuffer,
                              aSeeds: DeviceBuffer, errorSeeds: DeviceBuffer, out: DeviceBuffer, hashes: DeviceBuffer? = nil,
                              on stream: HeAmdStream) throws
    {
        try heAmdCheck(he_keyword_client_generate_query_device(context, wordBits, dimensions, UInt32(dimensions.count), entryCount,
                                                               entrySizeInBytes, hashFunctionCount, bytes(keywords),
                                                               words(keywordOffsets), queries, secretKey.pointer, bytes(aSeeds),
                                                               bytes(errorSeeds), out.pointer, hashes.map(words), nil, 0,
                                                               stream.raw))
    }

    /// `decrypt(response:at:using:)`: `response` [queries][h][R][2][moduliCount][N] and the keyword hashes `generateQuery` gave
    /// -> `values` [queries][valueCapacity], `sizes` uint64 [queries], `status` uint32 [queries] (`Status`).
    public func decrypt(response: DeviceBuffer, moduliCount: Int = 1, hashes: DeviceBuffer, queries: Int, secretKey: DeviceBuffer,
                        values: DeviceBuffer, sizes: DeviceBuffer, status: DeviceBuffer, on stream: HeAmdStream) throws
    {
        let outStatus = UnsafeMutableRawPointer(status.pointer).assumingMemoryBound(to: UInt32.self)
        try heAmdCheck(he_keyword_client_decrypt_response_device(context, wordBits, dimensions, UInt32(dimensions.count),
                                                                 entryCount, entrySizeInBytes, hashFunctionCount,
                                                                 UInt32(moduliCount), response.pointer, nil, nil, words(hashes),
                                                                 queries, secretKey.pointer, bytes(values), words(sizes),
                                                                 outStatus, nil, 0, stream.raw))
    }

    /// `countEntriesInResponse` per query: `counts` uint64 [queries].
    public func countEntries(response: DeviceBuffer, moduliCount: Int = 1, queries: Int, secretKey: DeviceBuffer,
                             counts: DeviceBuffer, on stream: HeAmdStream) throws
    {
        try heAmdCheck(he_keyword_client_count_entries_device(context, wordBits, dimensions, UInt32(dimensions.count), entryCount,
                                                              entrySizeInBytes, hashFunctionCount, UInt32(moduliCount),
                                                              response.pointer, queries, secretKey.pointer, words(counts), nil, 0,
                                                              stream.raw))
    }
}
