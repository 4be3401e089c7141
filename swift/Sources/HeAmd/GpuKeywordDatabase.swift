// KeywordDatabase.init(rows:sharding:shardingFunction:) on the device (reference Sources/PrivateInformationRetrieval/
// KeywordPir/KeywordDatabase.swift:406-437): the keyword and value bytes go up once, the device hashes the keywords, derives
// the shard indices and splits the rows (he_keyword_database_create_device), and every shard that received a row is a cuckoo
// table over the partitioned bytes -- the `table` and `values` arguments of he_keyword_pir_process_database_device, which
// builds the shard's index-PIR database (KeywordPirProtocol.swift:191-247).
import CHeAmd
import HomomorphicEncryption

/// One shard of a `GpuKeywordDatabase`: what `ProcessKeywordDatabase.processShard` is handed, resident on the device.
public struct GpuKeywordDatabaseShard {
    /// `KeywordDatabaseShard.shardID`: the decimal shard index (KeywordDatabase.swift:424).
    public let shardID: String
    /// Rows of the shard, duplicates included.
    public let rowCount: Int
    /// The shard's cuckoo table; owned by the database.
    public let table: OpaquePointer
    /// The shard's values, back to back in input order; owned by the database.
    public let values: UnsafePointer<UInt8>?
}

/// `KeywordDatabase` on the device.  `shards` lists the shards that received a row, as the reference's dictionary holds no
/// other (KeywordDatabase.swift:423).
public final class GpuKeywordDatabase: @unchecked Sendable {
    private let handle: OpaquePointer
    public let shardCount: Int
    public let shards: [GpuKeywordDatabaseShard]

    /// `Sharding.shardCount(for:)` with `Sharding.init`'s checks (KeywordDatabase.swift:186-204, :252-267).
    public static func shardCount(sharding: he_keyword_sharding, rowCount: Int) throws -> Int {
        var sharding = sharding
        var count = 0
        try heAmdCheck(he_keyword_sharding_shard_count(&sharding, rowCount, &count))
        return count
    }

    /// - Parameters:
    ///   - keywords, values: row i is (`keywords[i]`, `values[i]`), `KeywordValuePair` by `KeywordValuePair`.
    ///   - config: `CuckooTableConfig` as the C header states it.
    ///   - shardCount: the resolved shard count (`shardCount(sharding:rowCount:)`).
    ///   - otherShardCount: nonzero for `ShardingFunction.doubleMod(otherShardCount:)`, zero for `.sha256`.
    ///   - seed: shard s places its entries with seed + s.
    public init(keywords: [[UInt8]], values: [[UInt8]], config: he_cuckoo_table_config, shardCount: Int,
                otherShardCount: UInt64 = 0, seed: UInt64 = 0, on stream: HeAmdStream) throws
    {
        precondition(keywords.count == values.count)
        let rowCount = keywords.count
        var keywordOffsets = [UInt64](repeating: 0, count: rowCount + 1)
        var valueOffsets = [UInt64](repeating: 0, count: rowCount + 1)
        var keywordBytes: [UInt8] = []
        var valueBytes: [UInt8] = []
        for row in 0..<rowCount {
            keywordBytes.append(contentsOf: keywords[row])
            valueBytes.append(contentsOf: values[row])
            keywordOffsets[row + 1] = UInt64(keywordBytes.count)
            valueOffsets[row + 1] = UInt64(valueBytes.count)
        }
        // the bytes cross once, as they are; the object keeps its own partitioned copy, so these are freed on return
        let keywordWords = (keywordBytes.count + 7) / 8, valueWords = (valueBytes.count + 7) / 8
        let blobs = try DeviceBuffer(count: keywordWords + valueWords)
        try keywordBytes.withUnsafeBufferPointer { bytes in try blobs.upload(bytes: bytes, atByte: 0, on: stream) }
        try valueBytes.withUnsafeBufferPointer { bytes in try blobs.upload(bytes: bytes, atByte: keywordWords * 8, on: stream) }
        let keywordBlob = UnsafeRawPointer(blobs.pointer).assumingMemoryBound(to: UInt8.self)
        var config = config
        var created: OpaquePointer?
        try heAmdCheck(he_keyword_database_create_device(&config, keywordBlob, keywordOffsets, keywordBlob + keywordWords * 8,
                                                         valueOffsets, rowCount, shardCount, otherShardCount, seed, &created,
                                                         stream.raw))
        guard let created else { throw HeError.unsupportedHeOperation(description: "he_keyword_database_create_device returned nil") }
        handle = created
        self.shardCount = he_keyword_database_shard_count(created)
        var found: [GpuKeywordDatabaseShard] = []
        for shard in 0..<self.shardCount {
            guard let table = he_keyword_database_shard_table(created, shard) else { continue }
            found.append(GpuKeywordDatabaseShard(shardID: String(shard),
                                                 rowCount: he_keyword_database_shard_row_count(created, shard), table: table,
                                                 values: he_keyword_database_shard_values(created, shard)))
        }
        shards = found
    }

    deinit {
        he_keyword_database_destroy(handle)
    }

    /// Shard after shard, the input rows each holds.
    public func order() throws -> [UInt32] {
        var rows = [UInt32](repeating: 0, count: shards.reduce(0) { $0 + $1.rowCount })
        try heAmdCheck(he_keyword_database_order(handle, &rows))
        return rows
    }

    /// `KeywordPirServer.process` of one shard (KeywordPirProtocol.swift:220-239): the index-PIR database of every sub-table
    /// into `database` ([tableCount][chunks][prod(dimensions)][L][N] words) and `present`, both on the device.
    public func process(shard: GpuKeywordDatabaseShard, context: OpaquePointer, dimensions: [UInt32], entrySizeInBytes: Int,
                        database: DeviceBuffer, present: DeviceBuffer, on stream: HeAmdStream) throws
    {
        let mask = UnsafeMutableRawPointer(present.pointer).assumingMemoryBound(to: UInt8.self)
        try heAmdCheck(he_keyword_pir_process_database_device(context, shard.table, shard.values, dimensions,
                                                              UInt32(dimensions.count), entrySizeInBytes, database.pointer, mask,
                                                              stream.raw))
    }
}
